// rb_direct.hip -- direct light at surface points (rb_scene_emitters, rb_light_rays, rb_direct_light; DESIGN.md section 21, the
// normative definition): the scene's emitter table by an order-preserving compaction -- flag, exclusive scan, scatter -- over the
// raw scene arrays; the shadow ray of every (surfel, sample) item towards a point drawn on a uniformly picked emitter, with its
// bound and its unoccluded contribution; and the ordered sum of a surfel's contributions under the any-hit bytes of those rays.
// Beside the uniform pick, the pick by a table of integer weights (rb_emitter_cdf, rb_light_rays_cdf, rb_direct_light_cdf;
// section 23): the table by power -- every record's power and their maximum, the quantised weights, an inclusive scan -- and the
// same item with the emitter found in a table by a halving search.
// And the pick per grid cell (rb_emitter_grid_cdf, rb_light_rays_grid, rb_direct_light_grid; section 24): one such table per
// cell of a regular grid, weighted by power over squared distance to the cell, and the item searching the row of its surfel's cell.
// And the tables that learn visibility (rb_direct_light_grid_tally, rb_emitter_grid_learned; section 25): a count per (cell,
// emitter) of shadow rays tried and seen, kept by integer atomics behind the walk, and section 24's weight times the seen share.
// The generator runs before the kernels that walk the records (k_occl*, rb_query.hip), as k_hemi_rays does (section 16).  Same
// numerics contract as rb_kernels.hip: every step one binary32 operation in the order written, no FMA contraction, correctly
// rounded / and sqrt, so that renderbaby_amd/direct.py equals this file bit for bit.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include <rocprim/device/device_scan.hpp>

#include "rb_device_sincos.hpp"

#pragma clang fp contract(off)

namespace rb {
namespace {

DEV bool finite1(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }

// ===================================================== the emitter table ====
// Candidate i of the scene, in the table's order: triangles t < n_tris, then spheres, then lights.  The record is written whole
// whether or not the candidate qualifies; `ok` says whether it does (section 21.1).
struct Candidate {
    v4f q0, q1, q2, q3;   // the rb_emitter as four quads
    bool ok;
};
DEV Candidate emit_candidate(const EmitArgs& s, uint32_t i) {
    Candidate r;
    f3 a, b, c = mk(0, 0, 0), em = mk(0, 0, 0);
    uint32_t kind, prim;
    float area;
    bool geom;
    if (i < s.n_tris) {
        kind = RB_HIT_TRIANGLE;
        prim = i;
        const v4f* const t = reinterpret_cast<const v4f*>(s.tris + i);
        const v4f t0 = t[0], t1 = t[1], t2 = t[2];
        const uint32_t mesh = reinterpret_cast<const uint32_t*>(s.tris + i)[12];
        a = mk(t0.x, t0.y, t0.z);
        b = mk(t1.x, t1.y, t1.z) - a;
        c = mk(t2.x, t2.y, t2.z) - a;
        const f3 cr = cross(b, c);
        area = 0.5f * sqrt_exact((cr.x * cr.x + cr.y * cr.y) + cr.z * cr.z);
        geom = mesh < s.n_meshes;
        // rb_cast_rays' emissive of a triangle hit: the mesh's material, or nothing under the colour hash
        if (geom && s.color_hash == 0u) em = ld3(s.meshes[mesh].material.emissive);
    } else {
        const bool sphere = i - s.n_tris < s.n_spheres;
        kind = sphere ? RB_HIT_SPHERE : RB_HIT_LIGHT;
        prim = sphere ? i - s.n_tris : i - s.n_tris - s.n_spheres;
        // rb_sphere and rb_point_light share their layout: {centre, radius | material}
        const rb_sphere* const rec = sphere ? s.spheres + prim : reinterpret_cast<const rb_sphere*>(s.lights + prim);
        const v4f cr = reinterpret_cast<const v4f*>(rec)[0];
        a = mk(cr.x, cr.y, cr.z);
        b = mk(cr.w, 0.0f, 0.0f);
        area = 12.566371f * (cr.w * cr.w);
        geom = cr.w > 0.0f;
        em = ld3(rec->material.emissive);
    }
    r.ok = geom && finite3(em) && fmaxf(fmaxf(em.x, em.y), em.z) > 0.0f && finite3(a) && finite3(b) && finite3(c) && finite1(area) && area > 0.0f;
    r.q0 = v4f{a.x, a.y, a.z, __uint_as_float(kind)};
    r.q1 = v4f{b.x, b.y, b.z, __uint_as_float(prim)};
    r.q2 = v4f{c.x, c.y, c.z, area};
    r.q3 = v4f{em.x, em.y, em.z, 0.0f};
    return r;
}

__global__ void __launch_bounds__(256) k_emit_flag(const EmitArgs s, uint32_t total, uint32_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < total) flags[i] = emit_candidate(s, i).ok ? 1u : 0u;
}

// candidate i goes to out[offs[i]] if it qualifies and the table has room; the last lane leaves the total
__global__ void __launch_bounds__(256) k_emit_scatter(const EmitArgs s, uint32_t total, const uint32_t* __restrict__ flags,
                                                      const uint32_t* __restrict__ offs, rb_emitter* __restrict__ out, uint32_t capacity,
                                                      uint32_t* __restrict__ count) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const uint32_t off = offs[i], flag = flags[i];
    if (count != nullptr && i == total - 1u) *count = off + flag;
    if (flag == 0u || off >= capacity) return;
    const Candidate r = emit_candidate(s, i);
    v4f* const o = reinterpret_cast<v4f*>(out + off);
    o[0] = r.q0;
    o[1] = r.q1;
    o[2] = r.q2;
    o[3] = r.q3;
}

// ======================================================== k_light_rays ====
// lane = item, in k_hemi_rays' two orders (gen_item).  Item order (the engine's scratch): item = (block * samples + sample) * 64 +
// surfel-in-block, so that the fold's lanes -- one per surfel -- read a sample row as contiguous bytes, bounds and colours; the
// padding of the last block is written as invalid items, since k_occl* walk every record of the piece.  Linear order
// (rb_light_rays): item = surfel-in-piece * samples + sample.
// The lanes of a wave hold 64 different emitters: each lane fetches its own 64-byte record as four 16-byte loads (a record is
// one whole 64-byte segment, so no fetched byte is wasted), and the triangle and sphere arms are a branch, not selects -- a
// table of one kind, which is the common one (a mesh's emissive quads, or lamps only), then pays for one arm, and a mixed wave
// pays for both either way (section 21.3; argued from the instruction counts, not measured against selects).
// The item is defined once, light_item, for both picks (sections 21.1 and 23.1).  kCdf: the emitter comes from the inclusive
// table cdf[N] of pick weights and the factor is float(Q) / float(q) where the uniform pick has float(N).  The table's total Q
// = cdf[N - 1] is one address for the whole launch, so its test is wave-uniform; the search is up to 24 dependent 4-byte loads
// per lane from a table that lives in L2, each lane at its own place (the draws are independent), and it reads inside the table
// whatever the table holds: lo + len <= N and 1 <= half <= len - 1 throughout.  An item that the table leaves without a pick
// (Q == 0, Q > 2^24, or q == 0 from a malformed table) is what an item of an empty table is: dark, with the direction 0 0 0.
// kPick == PICK_GRID (section 24): `cdf` holds one such table per grid cell, row after row, and a valid item searches the row
// of the cell its surfel's position falls into -- the nearest cell for a point outside the grid --, so Q is per lane.  In item
// order the 64 lanes of a wave are 64 neighbouring surfels of one sample and mostly share a row.  row < rows for every float
// the position holds, and the search stays inside its row as it stays inside the one table: every index read is in
// [0, rows * N - 1] whatever the tables hold.  An invalid item reads row 0's total and nothing else.
enum PickMode { PICK_UNIFORM, PICK_CDF, PICK_GRID };

// the cell of section 24 along one axis: min((uint32_t)max(f, 0.0f), count - 1), the conversion truncating and saturating; f is
// no NaN (a valid surfel's position and the grid's origin are finite, the step is finite and above 0)
DEV uint32_t grid_axis(float pos, float origin, float step, uint32_t count) {
    const float f = fmaxf((pos - origin) / step, 0.0f);
    return f >= 4294967296.0f ? count - 1u : min((uint32_t)f, count - 1u);
}

// The pick from a table (sections 23.1 and 24.1), once for the generator and for the count of section 25: the row a valid
// item's position searches (PICK_GRID; `row` stays 0 otherwise), Q, the halving search, q and the factor float(Q) / float(q).
// Returns whether the item has a pick; an invalid item reads the total of the table's first row and nothing else.
template <PickMode kPick>
DEV bool table_pick(const uint32_t* __restrict__ cdf, const rb_probe_grid* grid, uint32_t N, bool valid, f3 pos, float u0, uint32_t& row,
                    uint32_t& j, float& fn) {
    if constexpr (kPick == PICK_GRID) {
        if (valid) {
            const uint32_t ix = grid_axis(pos.x, grid->origin[0], grid->step[0], grid->counts[0]);
            const uint32_t iy = grid_axis(pos.y, grid->origin[1], grid->step[1], grid->counts[1]);
            const uint32_t iz = grid_axis(pos.z, grid->origin[2], grid->step[2], grid->counts[2]);
            row = (iz * grid->counts[1] + iy) * grid->counts[0] + ix;
            cdf += (size_t)row * N;   // rows * N <= RB_MAX_GRID_ENTRIES
        }
    }
    const uint32_t Q = N != 0u ? cdf[N - 1u] : 0u;
    bool picked = Q != 0u && Q <= (1u << 24);
    if (valid && picked) {
        const float fq = (float)Q;   // Q <= 2^24: exact
        const uint32_t tq = min((uint32_t)(u0 * fq), Q - 1u);
        uint32_t lo = 0u, len = N;
        while (len > 1u) {
            const uint32_t half = len >> 1;
            if (cdf[lo + half - 1u] <= tq) {
                lo += half;
                len -= half;
            } else {
                len = half;
            }
        }
        j = lo;
        const uint32_t q = cdf[j] - (j != 0u ? cdf[j - 1u] : 0u);
        picked = q != 0u;
        fn = fq / (float)q;
    }
    return picked;
}

template <PickMode kPick>
DEV void light_item(const LightGenArgs g, const uint32_t* __restrict__ cdf, const rb_probe_grid* grid = nullptr) {
    constexpr bool kCdf = kPick != PICK_UNIFORM;
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const GenItem it = gen_item(t, g.samples, g.linear);
    const uint32_t sf = it.idx, smp = it.smp;
    if (sf >= g.n) {
        // linear order: the lanes behind the last item; item order: those, and the padding of the last block
        if (g.linear != 0u || sf >= ((g.n + 63u) & ~63u)) return;
        store_record(g.recs, nullptr, t, mk(0, 0, 0), mk(0, 0, 0), 0u);
        g.tmax[t] = 0.0f;
        reinterpret_cast<v4f*>(g.contrib)[t] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
        return;
    }

    const v4f* const sp = reinterpret_cast<const v4f*>(g.surfels) + (size_t)sf * 2u;
    const v4f s0 = sp[0], s1 = sp[1];
    const f3 pos = mk(s0.x, s0.y, s0.z);
    const f3 nrm = normalize(mk(s1.x, s1.y, s1.z));
    const float reach = sqrt_exact((pos.x * pos.x + pos.y * pos.y) + pos.z * pos.z);
    f3 o = pos + (g.offset * fmaxf(1.0f, reach)) * nrm;
    const bool valid = finite3(pos) && finite3(nrm) && !zero3(nrm) && finite3(o);

    const uint32_t sid = g.ids != nullptr ? g.ids[sf] : g.id_base + sf;
    uint32_t seed = pcg(sid + pcg(g.first_sample + smp));
    const float u0 = rnd(seed), u1 = rnd(seed), u2 = rnd(seed);

    const uint32_t N = g.n_emit;
    f3 d = mk(0, 0, 0);
    float tmax = 0.0f;
    v4f contrib = v4f{0.0f, 0.0f, 0.0f, valid ? 1.0f : 0.0f};
    uint32_t j = 0u;
    float fn = 0.0f;       // the factor: float(N), or float(Q) / float(q)
    bool picked = N != 0u;
    if constexpr (kCdf) {
        uint32_t row = 0u;
        picked = table_pick<kPick>(cdf, grid, N, valid, pos, u0, row, j, fn);
    }
    if (valid && picked) {
        if constexpr (!kCdf) {
            fn = (float)N;   // N <= 2^24: exact
            j = min((uint32_t)(u0 * fn), N - 1u);
        }
        const v4f* const ep = reinterpret_cast<const v4f*>(g.emitters) + (size_t)j * 4u;
        const v4f e0 = ep[0], e1 = ep[1], e2 = ep[2], e3 = ep[3];
        const f3 a = mk(e0.x, e0.y, e0.z), b = mk(e1.x, e1.y, e1.z), c = mk(e2.x, e2.y, e2.z), em = mk(e3.x, e3.y, e3.z);
        const uint32_t kind = __float_as_uint(e0.w);
        const float area = e2.w;
        const bool good = finite3(a) && finite3(b) && finite3(c) && finite3(em) && finite1(area) && area > 0.0f &&
                          (kind == (uint32_t)RB_HIT_TRIANGLE || kind == (uint32_t)RB_HIT_SPHERE || kind == (uint32_t)RB_HIT_LIGHT);
        f3 Q, ne;
        if (kind == (uint32_t)RB_HIT_TRIANGLE) {
            const float su = sqrt_exact(u1);
            const float bv = u2 * su;
            const float bu = su - bv;
            Q = (a + bu * b) + bv * c;
            ne = normalize(cross(b, c));
        } else {
            const SinCos az = sincos_turn(u1 * 2.0f - 1.0f);
            const float z = 1.0f - (u2 + u2);
            const float r = sqrt_exact(1.0f - z * z);   // |z| <= 1: the radicand is >= 0
            ne = mk(r * az.c, r * az.s, z);
            Q = a + b.x * ne;
        }
        const f3 v = Q - o;
        const float d2 = (v.x * v.x + v.y * v.y) + v.z * v.z;
        const float dist = sqrt_exact(d2);
        d = divs(v, dist);
        const float cs = dot(nrm, d);
        float ce = dot(ne, d);
        ce = kind == (uint32_t)RB_HIT_TRIANGLE ? fabsf(ce) : -ce;
        // a NaN made here has no defined sign or payload and stays out of the record
        const bool aimed = finite3(d) && !zero3(d);
        if (!aimed) d = mk(0, 0, 0);
        if (good && aimed && cs > 0.0f && ce > 0.0f && d2 > 0.0f) {
            const float gm = ((((cs * ce) * area) / d2) * fn) * 0.318309886f;
            const f3 lit = mk(em.x * gm, em.y * gm, em.z * gm);
            if (finite3(lit)) {
                contrib = v4f{lit.x, lit.y, lit.z, 1.0f};
                tmax = dist * (1.0f - g.shorten);
            }
        }
    }
    if (!valid) o = pos;   // an invalid item keeps the surfel's position as it was given beside a zero direction

    store_record(g.recs, nullptr, t, o, d, 0u);
    g.tmax[t] = tmax;
    reinterpret_cast<v4f*>(g.contrib)[t] = contrib;
}

__global__ void __launch_bounds__(256) k_light_rays(const LightGenArgs g) { light_item<PICK_UNIFORM>(g, nullptr); }
__global__ void __launch_bounds__(256) k_light_rays_cdf(const LightGenArgs g, const uint32_t* __restrict__ cdf) { light_item<PICK_CDF>(g, cdf); }
__global__ void __launch_bounds__(256) k_light_rays_grid(const LightGenArgs g, const uint32_t* __restrict__ tables, const rb_probe_grid grid) {
    light_item<PICK_GRID>(g, tables, &grid);
}

// ================================================= the table by power ====
// p_j of section 23.1 for every record, and the largest of them folded into *pmax (zeroed before the launch): p >= 0, so the
// floats order as their bit patterns do and the maximum is an integer one -- exact, whatever order the atomics arrive in.
DEV float emit_power(const rb_emitter* __restrict__ em, uint32_t j) {
    const v4f* const ep = reinterpret_cast<const v4f*>(em) + (size_t)j * 4u;
    const v4f e0 = ep[0], e1 = ep[1], e2 = ep[2], e3 = ep[3];
    const f3 a = mk(e0.x, e0.y, e0.z), b = mk(e1.x, e1.y, e1.z), c = mk(e2.x, e2.y, e2.z), em3 = mk(e3.x, e3.y, e3.z);
    const uint32_t kind = __float_as_uint(e0.w);
    const float area = e2.w;
    const bool good = finite3(a) && finite3(b) && finite3(c) && finite3(em3) && finite1(area) && area > 0.0f &&
                      (kind == (uint32_t)RB_HIT_TRIANGLE || kind == (uint32_t)RB_HIT_SPHERE || kind == (uint32_t)RB_HIT_LIGHT);
    const float m = fmaxf(fmaxf(em3.x, em3.y), em3.z);
    const float p = fminf(m * area, 3.4028235e38f);
    return (good && m > 0.0f && p > 0.0f) ? p : 0.0f;
}

__global__ void __launch_bounds__(256) k_emit_power(const rb_emitter* __restrict__ em, uint32_t n, float* __restrict__ power,
                                                    uint32_t* __restrict__ pmax) {
    __shared__ uint32_t block_max;
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (threadIdx.x == 0u) block_max = 0u;
    __syncthreads();
    float p = 0.0f;
    if (j < n) {
        p = emit_power(em, j);
        power[j] = p;
    }
    uint32_t bits = __float_as_uint(p);
    for (int off = 32; off > 0; off >>= 1) bits = max(bits, (uint32_t)__shfl_xor((int)bits, off, 64));
    if ((threadIdx.x & 63u) == 0u && bits != 0u) atomicMax(&block_max, bits);
    __syncthreads();
    if (threadIdx.x == 0u && block_max != 0u) atomicMax(pmax, block_max);
}

// q_j = p_j > 0 ? max(1, uint((p_j / pmax) * float(S))) : 0; pmax == 0: every p is 0
__global__ void __launch_bounds__(256) k_emit_quant(const float* __restrict__ power, const uint32_t* __restrict__ pmax, uint32_t n,
                                                    float scale, uint32_t* __restrict__ q) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const float p = power[j], top = __uint_as_float(*pmax);
    q[j] = p > 0.0f ? max(1u, (uint32_t)((p / top) * scale)) : 0u;
}

// ================================================= the tables per cell ====
// {ce, re} of section 24 for every record, beside k_emit_power's p: a sphere that holds the emitter.  A record that is not good
// has p = 0 and its bound is never looked at.
__global__ void __launch_bounds__(256) k_emit_bound(const rb_emitter* __restrict__ em, uint32_t n, v4f* __restrict__ bound) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const v4f* const ep = reinterpret_cast<const v4f*>(em) + (size_t)j * 4u;
    const v4f e0 = ep[0], e1 = ep[1], e2 = ep[2];
    const f3 a = mk(e0.x, e0.y, e0.z), b = mk(e1.x, e1.y, e1.z), c = mk(e2.x, e2.y, e2.z);
    f3 ce = a;
    float re = fabsf(b.x);
    if (__float_as_uint(e0.w) == (uint32_t)RB_HIT_TRIANGLE) {
        ce = a + 0.33333334f * (b + c);
        const f3 v0 = a - ce, v1 = (a + b) - ce, v2 = (a + c) - ce;
        const float l0 = (v0.x * v0.x + v0.y * v0.y) + v0.z * v0.z;
        const float l1 = (v1.x * v1.x + v1.y * v1.y) + v1.z * v1.z;
        const float l2 = (v2.x * v2.x + v2.y * v2.y) + v2.z * v2.z;
        const float m01 = l0 > l1 ? l0 : l1;
        re = sqrt_exact(m01 > l2 ? m01 : l2);
    }
    bound[j] = v4f{ce.x, ce.y, ce.z, re};
}

// w of section 24: the power over the squared distance from the cell's centre to the bound's centre, no nearer than the two
// radii together.  max and min are `x > y ? x : y` and `x < y ? x : y`, so w is in [0, 3.4028235e38] -- never a NaN -- whatever
// the bound holds, and the floats order as their bit patterns do.
DEV float grid_weight(v4f bnd, float p, f3 cc, float hd) {
    const f3 v = mk(bnd.x, bnd.y, bnd.z) - cc;
    const float d2 = (v.x * v.x + v.y * v.y) + v.z * v.z;
    const float r0 = bnd.w + hd;
    const float fl = r0 * r0;
    const float x = p / (d2 > fl ? d2 : fl);
    const float w = x < 3.4028235e38f ? x : 3.4028235e38f;
    return p > 0.0f ? w : 0.0f;
}

// One block per cell, row = blockIdx.x, and GRID_CHUNK entries of its row per step.  Sweep 1: the row's largest weight, folded
// on the bit pattern over the wave and through one LDS word.  Sweep 2: w again from the record's 20 bytes (L2 holds them; a
// rows * N float scratch would cost a global round trip more than it saves), q, and the inclusive sums chunk by chunk -- a wave
// scan by lane shuffles, the four waves joined through LDS, the chunk's total carried into the next.  Integer sums: the row
// does not depend on the scan's shape.  The row is the only global write, 4 B per lane, coalesced.
// kSeen (section 25): w' = w f in both sweeps, f from the 8-byte record of (row, j) in the caller's tally and the prior.
constexpr uint32_t GRID_CHUNK = 256u;

// f of section 25: ((float)s + a) / ((float)t + a) with s = min(seen, tried); in [0, 1], never a NaN, for 0 < a <= 2^24
DEV float seen_share(const uint32_t* __restrict__ rec, float prior) {   // two 4-byte loads: the tally is 4-byte aligned
    const uint32_t t = rec[0], s = min(rec[1], t);
    return ((float)s + prior) / ((float)t + prior);
}

template <bool kSeen>
DEV void grid_rows(const v4f* __restrict__ bound, const float* __restrict__ power, uint32_t n, const rb_probe_grid& grid, float scale,
                   uint32_t* __restrict__ tables, const uint32_t* __restrict__ tally, float prior) {
    __shared__ uint32_t row_max;
    __shared__ uint32_t wave_sum[4];
    const uint32_t row = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nx = grid.counts[0], ny = grid.counts[1];
    const uint32_t ix = row % nx, iy = (row / nx) % ny, iz = row / (nx * ny);
    const f3 cc = mk(grid.origin[0] + ((float)ix + 0.5f) * grid.step[0], grid.origin[1] + ((float)iy + 0.5f) * grid.step[1],
                     grid.origin[2] + ((float)iz + 0.5f) * grid.step[2]);
    const float sx = grid.step[0], sy = grid.step[1], sz = grid.step[2];
    const float hd = sqrt_exact(0.25f * ((sx * sx + sy * sy) + sz * sz));

    if (tid == 0u) row_max = 0u;
    __syncthreads();
    uint32_t bits = 0u;
    if constexpr (kSeen) tally += (size_t)row * n * 2u;   // rows * n <= RB_MAX_GRID_ENTRIES records
    for (uint32_t j = tid; j < n; j += GRID_CHUNK) {
        float w = grid_weight(bound[j], power[j], cc, hd);
        if constexpr (kSeen) w = w * seen_share(tally + (size_t)j * 2u, prior);
        bits = max(bits, __float_as_uint(w));
    }
    for (int off = 32; off > 0; off >>= 1) bits = max(bits, (uint32_t)__shfl_xor((int)bits, off, 64));
    if (lane == 0u && bits != 0u) atomicMax(&row_max, bits);
    __syncthreads();
    const float wmax = __uint_as_float(row_max);

    uint32_t* const out = tables + (size_t)row * n;
    uint32_t carry = 0u;
    for (uint32_t base = 0u; base < n; base += GRID_CHUNK) {   // (n <= 2^24: base + tid does not wrap)
        const uint32_t j = base + tid;
        uint32_t q = 0u;
        if (j < n) {
            const float p = power[j];
            if (p > 0.0f) {
                float w = grid_weight(bound[j], p, cc, hd);
                if constexpr (kSeen) w = w * seen_share(tally + (size_t)j * 2u, prior);
                q = wmax > 0.0f ? max(1u, (uint32_t)((w / wmax) * scale)) : 1u;
            }
        }
        uint32_t sum = q;
        for (uint32_t off = 1u; off < 64u; off <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)sum, off, 64);
            if (lane >= off) sum += up;
        }
        if (lane == 63u) wave_sum[wave] = sum;
        __syncthreads();
        const uint32_t s0 = wave_sum[0], s1 = wave_sum[1], s2 = wave_sum[2], s3 = wave_sum[3];
        const uint32_t before = wave == 0u ? 0u : wave == 1u ? s0 : wave == 2u ? s0 + s1 : (s0 + s1) + s2;
        if (j < n) out[j] = (carry + before) + sum;
        carry += ((s0 + s1) + s2) + s3;
        __syncthreads();   // wave_sum is the next chunk's
    }
}

__global__ void __launch_bounds__(256) k_grid_rows(const v4f* __restrict__ bound, const float* __restrict__ power, uint32_t n,
                                                   const rb_probe_grid grid, float scale, uint32_t* __restrict__ tables) {
    grid_rows<false>(bound, power, n, grid, scale, tables, nullptr, 0.0f);
}
__global__ void __launch_bounds__(256) k_grid_rows_seen(const v4f* __restrict__ bound, const float* __restrict__ power, uint32_t n,
                                                        const rb_probe_grid grid, float scale, uint32_t* __restrict__ tables,
                                                        const uint32_t* __restrict__ tally, float prior) {
    grid_rows<true>(bound, power, n, grid, scale, tables, tally, prior);
}

// ========================================================= k_grid_tally ====
// The count of section 25, behind the walk: lane = surfel and the items of a surfel at k_direct_fold's places, in both orders.
// An item whose stored bound is > 0 was valid, picked and lit -- a real shadow ray --, and only such an item is looked at: its
// pick is made again from the surfel's position (the row, once per lane), the item's first draw and the row's search, which is
// the generator's own function on the same tables, so (row, j) is the record the ray was aimed at and row * N + j < rows * N
// whatever the tables hold.  Integer atomics in global memory whose old value nobody reads: the sums are exact in any order.
// The lanes of a wave are 64 neighbouring surfels of one sample and mostly share a row; how many share a record depends on the
// table (all 64 with one emitter), and atomics on one address are served one after another (section 25.5: 0.6 G adds/s on two
// emitters).  kCombine, the form that is launched: per sample the wave groups its counted lanes by record -- the first
// counted lane's record is broadcast, a ballot finds the lanes that share it, that lane adds the two popcounts, the group
// leaves the mask -- so a record gets one add per wave and sample, and the loop runs once per distinct record, 64 times at the
// most.  Every lane of a wave stays in the sample loop (its trip count is the launch's) so that the ballots see whole waves;
// a lane behind the last surfel counts nothing.  The plain form, one add per item, is kept for the measurement
// (RB_GRID_TALLY=plain); both give the same sums.
template <bool kCombine>
DEV void grid_tally(const LightGenArgs& g, const uint32_t* __restrict__ tables, const rb_probe_grid& grid, const uint8_t* __restrict__ occl,
                    uint32_t* __restrict__ tally) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    const bool live = i < g.n;
    const uint32_t S = g.samples, N = g.n_emit;
    const size_t row0 = g.linear != 0u ? (size_t)i * S : ((size_t)(i >> 6) * S) * 64u + (i & 63u);
    const size_t step = g.linear != 0u ? 1u : 64u;
    f3 pos = mk(0, 0, 0);
    uint32_t sid = 0u;
    if (live) {
        const v4f s0 = reinterpret_cast<const v4f*>(g.surfels)[(size_t)i * 2u];
        pos = mk(s0.x, s0.y, s0.z);
        sid = g.ids != nullptr ? g.ids[i] : g.id_base + i;
    }
    for (uint32_t s = 0; s < S; s++) {
        bool counted = false, visible = false;
        uint32_t key = 0u;   // row * N + j < 2^26
        if (live) {
            const size_t t = row0 + (size_t)s * step;
            if (g.tmax[t] > 0.0f) {
                uint32_t seed = pcg(sid + pcg(g.first_sample + s));
                const float u0 = rnd(seed);
                uint32_t row = 0u, j = 0u;
                float fn = 0.0f;
                counted = table_pick<PICK_GRID>(tables, &grid, N, true, pos, u0, row, j, fn);   // (false: tables changed under the call)
                key = row * N + j;
                visible = occl[t] == (uint8_t)RB_OCCL_VISIBLE;
            }
        }
        if constexpr (kCombine) {
            unsigned long long todo = __ballot(counted);
            while (todo != 0ull) {   // wave-uniform: every lane holds the same mask
                const int leader = __ffsll(todo) - 1;
                const uint32_t k = (uint32_t)__shfl((int)key, leader, 64);
                const bool mine = counted && key == k;
                const unsigned long long same = __ballot(mine), seen = __ballot(mine && visible);
                if (lane == (uint32_t)leader) {
                    atomicAdd(tally + (size_t)k * 2u, (uint32_t)__popcll(same));
                    if (seen != 0ull) atomicAdd(tally + (size_t)k * 2u + 1u, (uint32_t)__popcll(seen));
                }
                todo &= ~same;   // the leader is in `same`: the loop ends
            }
        } else if (counted) {
            atomicAdd(tally + (size_t)key * 2u, 1u);
            if (visible) atomicAdd(tally + (size_t)key * 2u + 1u, 1u);
        }
    }
}

__global__ void __launch_bounds__(256) k_grid_tally(const LightGenArgs g, const uint32_t* __restrict__ tables, const rb_probe_grid grid,
                                                    const uint8_t* __restrict__ occl, uint32_t* __restrict__ tally) {
    grid_tally<true>(g, tables, grid, occl, tally);
}
__global__ void __launch_bounds__(256) k_grid_tally_plain(const LightGenArgs g, const uint32_t* __restrict__ tables, const rb_probe_grid grid,
                                                          const uint8_t* __restrict__ occl, uint32_t* __restrict__ tally) {
    grid_tally<false>(g, tables, grid, occl, tally);
}

// ======================================================= k_direct_fold ====
// lane = surfel, a block of 64 surfels per wavefront as k_rad_sum has it: sample row s of the block is 64 contiguous result
// bytes and 1 KiB of colours.  `linear`: the items lie surfel by surfel instead (a piece of fewer than 64 surfels, which would
// otherwise be padded to a whole block).  From +0, in ascending sample order: the colour of every item whose byte is RB_OCCL_VISIBLE, one
// add per component; the weight is the sum of the items' fourth words (1 = a valid item).
__global__ void __launch_bounds__(256) k_direct_fold(const uint8_t* __restrict__ occl, const float* __restrict__ contrib, uint32_t n,
                                                     uint32_t S, uint32_t linear, rb_radiance* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const size_t row0 = linear != 0u ? (size_t)i * S : ((size_t)(i >> 6) * S) * 64u + (i & 63u);
    const size_t step = linear != 0u ? 1u : 64u;
    const uint8_t* const ob = occl + row0;
    const v4f* const cb = reinterpret_cast<const v4f*>(contrib) + row0;
    float r = 0.0f, gr = 0.0f, b = 0.0f, w = 0.0f;
    for (uint32_t s = 0; s < S; s++) {
        const uint32_t byte = ob[(size_t)s * step];
        const v4f c = cb[(size_t)s * step];
        if (byte == (uint32_t)RB_OCCL_VISIBLE) {
            r = r + c.x;
            gr = gr + c.y;
            b = b + c.z;
        }
        w = w + c.w;
    }
    reinterpret_cast<v4f*>(out)[i] = v4f{r, gr, b, w};
}

size_t align256(size_t x) { return (x + 255u) & ~size_t(255); }

hipError_t scan_bytes_for(uint32_t total, size_t* bytes) {
    *bytes = 0;
    return rocprim::exclusive_scan(nullptr, *bytes, static_cast<uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), 0u, total,
                                   rocprim::plus<uint32_t>(), static_cast<hipStream_t>(nullptr));
}

hipError_t cdf_scan_bytes_for(uint32_t n, size_t* bytes) {
    *bytes = 0;
    return rocprim::inclusive_scan(nullptr, *bytes, static_cast<uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), n, rocprim::plus<uint32_t>(),
                                   static_cast<hipStream_t>(nullptr));
}

}  // namespace

// the powers and the quantised weights of n records, the word of the largest power and the scan's own scratch behind them;
// 0: the scan could not be sized
size_t emitter_cdf_work_bytes(uint32_t n) {
    size_t scan = 0;
    if (n == 0u) return 256u;
    if (cdf_scan_bytes_for(n, &scan) != hipSuccess) return 0;
    return 2u * align256(4u * (size_t)n) + 256u + align256(scan) + 256u;
}

// cdf[n] of em[n] by power (section 23.1), queued on `stream`: the powers and their maximum, the quantised weights, their
// inclusive sums -- integers, so the scan's order does not show.  Nothing is waited for.
int launch_emitter_cdf(const rb_emitter* em, uint32_t n, void* work, uint32_t* cdf, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (n == 0u) return 0;
    if (em == nullptr || work == nullptr || cdf == nullptr || n > RB_MAX_EMITTERS) return (int)hipErrorInvalidValue;
    size_t scan = 0;
    if (const hipError_t st = cdf_scan_bytes_for(n, &scan)) return (int)st;
    char* const base = static_cast<char*>(work);
    float* const power = reinterpret_cast<float*>(base);
    uint32_t* const q = reinterpret_cast<uint32_t*>(base + align256(4u * (size_t)n));
    uint32_t* const pmax = reinterpret_cast<uint32_t*>(base + 2u * align256(4u * (size_t)n));
    void* const tmp = base + 2u * align256(4u * (size_t)n) + 256u;
    uint32_t L = 0u;
    while ((1u << L) < n) L++;
    const float scale = (float)(1u << (24u - L));
    if (const hipError_t st = hipMemsetAsync(pmax, 0, sizeof(uint32_t), stream)) return (int)st;
    hipLaunchKernelGGL(k_emit_power, dim3((n + 255u) / 256u), dim3(256), 0, stream, em, n, power, pmax);
    if (const hipError_t st = hipGetLastError()) return (int)st;
    hipLaunchKernelGGL(k_emit_quant, dim3((n + 255u) / 256u), dim3(256), 0, stream, power, pmax, n, scale, q);
    if (const hipError_t st = hipGetLastError()) return (int)st;
    return (int)rocprim::inclusive_scan(tmp, scan, q, cdf, n, rocprim::plus<uint32_t>(), stream);
}

// the powers, the word of their largest (k_emit_power's, not read here) and the bounds of n records
size_t emitter_grid_work_bytes(uint32_t n) { return align256(4u * (size_t)n) + 256u + align256(16u * (size_t)n) + 256u; }

// tables[rows * n] of em[n] over `grid` (section 24), queued on `stream`: the powers and the bounds, one lane per record, then
// one block per cell.  Nothing is waited for.  The caller has checked the grid and rows * n <= RB_MAX_GRID_ENTRIES.
// `tally`: rows * n records in device memory and a prior the caller has checked -- the learned weight of section 25 (k_grid_rows_seen)
int launch_emitter_grid(const rb_emitter* em, uint32_t n, const rb_probe_grid& grid, void* work, uint32_t* tables, void* stream_,
                        const rb_grid_tally* tally, float prior) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (n == 0u) return 0;
    const uint64_t rows = (uint64_t)grid.counts[0] * grid.counts[1] * grid.counts[2];
    if (em == nullptr || work == nullptr || tables == nullptr || n > RB_MAX_EMITTERS || rows == 0u || rows * n > RB_MAX_GRID_ENTRIES)
        return (int)hipErrorInvalidValue;
    char* const base = static_cast<char*>(work);
    float* const power = reinterpret_cast<float*>(base);
    uint32_t* const pmax = reinterpret_cast<uint32_t*>(base + align256(4u * (size_t)n));
    v4f* const bound = reinterpret_cast<v4f*>(base + align256(4u * (size_t)n) + 256u);
    uint32_t L = 0u;
    while ((1u << L) < n) L++;
    const float scale = (float)(1u << (24u - L));
    if (const hipError_t st = hipMemsetAsync(pmax, 0, sizeof(uint32_t), stream)) return (int)st;
    hipLaunchKernelGGL(k_emit_power, dim3((n + 255u) / 256u), dim3(256), 0, stream, em, n, power, pmax);
    if (const hipError_t st = hipGetLastError()) return (int)st;
    hipLaunchKernelGGL(k_emit_bound, dim3((n + 255u) / 256u), dim3(256), 0, stream, em, n, bound);
    if (const hipError_t st = hipGetLastError()) return (int)st;
    if (tally != nullptr)
        hipLaunchKernelGGL(k_grid_rows_seen, dim3((uint32_t)rows), dim3(256), 0, stream, bound, power, n, grid, scale, tables,
                           reinterpret_cast<const uint32_t*>(tally), prior);
    else
        hipLaunchKernelGGL(k_grid_rows, dim3((uint32_t)rows), dim3(256), 0, stream, bound, power, n, grid, scale, tables);
    return (int)hipGetLastError();
}

uint64_t emitter_candidates(const EmitArgs& s) { return (uint64_t)s.n_tris + s.n_spheres + s.n_lights; }

// flags and offsets of every candidate, the scan's own scratch behind them; 0: the scan could not be sized
size_t emitter_work_bytes(uint32_t total) {
    size_t scan = 0;
    if (scan_bytes_for(total, &scan) != hipSuccess) return 0;
    return 2u * align256(4u * (size_t)total) + align256(scan) + 256u;
}

// the flags and the exclusive offsets of the scene's candidates into `work`, and the number that qualify into *count
int launch_emitter_count(const EmitArgs& s, void* work, uint32_t* count, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const uint32_t total = (uint32_t)emitter_candidates(s);
    if (total == 0u) return (int)hipMemsetAsync(count, 0, sizeof(uint32_t), stream);
    size_t scan = 0;
    if (const hipError_t st = scan_bytes_for(total, &scan)) return (int)st;
    char* const base = static_cast<char*>(work);
    uint32_t* const flags = reinterpret_cast<uint32_t*>(base);
    uint32_t* const offs = reinterpret_cast<uint32_t*>(base + align256(4u * (size_t)total));
    void* const tmp = base + 2u * align256(4u * (size_t)total);
    hipLaunchKernelGGL(k_emit_flag, dim3((total + 255u) / 256u), dim3(256), 0, stream, s, total, flags);
    if (const hipError_t st = hipGetLastError()) return (int)st;
    if (const hipError_t st = rocprim::exclusive_scan(tmp, scan, flags, offs, 0u, total, rocprim::plus<uint32_t>(), stream)) return (int)st;
    // (no record is written: capacity 0)
    hipLaunchKernelGGL(k_emit_scatter, dim3((total + 255u) / 256u), dim3(256), 0, stream, s, total, flags, offs, static_cast<rb_emitter*>(nullptr), 0u, count);
    return (int)hipGetLastError();
}

// ... and the records of those that qualify, in candidate order, into out[capacity], from the flags and offsets `work` holds
int launch_emitter_scatter(const EmitArgs& s, const void* work, rb_emitter* out, uint32_t capacity, void* stream_) {
    const uint32_t total = (uint32_t)emitter_candidates(s);
    if (total == 0u || capacity == 0u) return 0;
    const char* const base = static_cast<const char*>(work);
    const uint32_t* const flags = reinterpret_cast<const uint32_t*>(base);
    const uint32_t* const offs = reinterpret_cast<const uint32_t*>(base + align256(4u * (size_t)total));
    hipLaunchKernelGGL(k_emit_scatter, dim3((total + 255u) / 256u), dim3(256), 0, static_cast<hipStream_t>(stream_), s, total, flags, offs, out, capacity,
                       static_cast<uint32_t*>(nullptr));
    return (int)hipGetLastError();
}

// One piece: every record, bound and colour of it, queued on `stream`; nothing is waited for.  Item order: g.n surfels rounded
// up to whole blocks of 64, the padding written as invalid items; linear order: g.n surfels' g.n * samples items.
// `cdf`: nullptr for the uniform pick (k_light_rays), or g.n_emit inclusive pick weights in device memory (k_light_rays_cdf);
// with `cells`, one such table per cell of that grid (k_light_rays_grid)
int launch_light_rays(const LightGenArgs& g, void* stream_, const uint32_t* cdf, const rb_probe_grid* cells) {
    if (g.n == 0u) return 0;
    if (g.surfels == nullptr || g.recs == nullptr || g.tmax == nullptr || g.contrib == nullptr || g.samples == 0u) return (int)hipErrorInvalidValue;
    if (g.emitters == nullptr && (g.n_emit != 0u)) return (int)hipErrorInvalidValue;
    if (g.n_emit > RB_MAX_EMITTERS) return (int)hipErrorInvalidValue;
    const uint64_t lanes = gen_lanes(g.n, g.samples, g.linear);
    if (lanes == 0u) return (int)hipErrorInvalidValue;
    const dim3 grid((uint32_t)((lanes + 255u) / 256u));
    if (cdf != nullptr && cells != nullptr && g.n_emit != 0u)
        hipLaunchKernelGGL(k_light_rays_grid, grid, dim3(256), 0, static_cast<hipStream_t>(stream_), g, cdf, *cells);
    else if (cdf != nullptr && g.n_emit != 0u)
        hipLaunchKernelGGL(k_light_rays_cdf, grid, dim3(256), 0, static_cast<hipStream_t>(stream_), g, cdf);
    else
        hipLaunchKernelGGL(k_light_rays, grid, dim3(256), 0, static_cast<hipStream_t>(stream_), g);
    return (int)hipGetLastError();
}

// The count of one piece behind its walk (section 25): g as the piece's generator had it, `tables` and `cells` its tables and
// grid, `occl` the walk's bytes beside g.tmax; adds into tally[rows * g.n_emit].  Queued, nothing is waited for.
int launch_grid_tally(const LightGenArgs& g, const uint32_t* tables, const rb_probe_grid& cells, const uint8_t* occl, rb_grid_tally* tally,
                      void* stream_) {
    if (g.n == 0u || g.n_emit == 0u) return 0;
    if (g.surfels == nullptr || g.tmax == nullptr || tables == nullptr || occl == nullptr || tally == nullptr || g.samples == 0u)
        return (int)hipErrorInvalidValue;
    const uint64_t rows = (uint64_t)cells.counts[0] * cells.counts[1] * cells.counts[2];
    if (g.n_emit > RB_MAX_EMITTERS || rows == 0u || rows * g.n_emit > RB_MAX_GRID_ENTRIES) return (int)hipErrorInvalidValue;
    if (gen_lanes(g.n, g.samples, g.linear) == 0u) return (int)hipErrorInvalidValue;
    const char* const form = std::getenv("RB_GRID_TALLY");   // "plain": one add per item, for the measurement of section 25.5
    if (form != nullptr && std::strcmp(form, "plain") == 0)
        hipLaunchKernelGGL(k_grid_tally_plain, dim3((g.n + 255u) / 256u), dim3(256), 0, static_cast<hipStream_t>(stream_), g, tables, cells, occl,
                           reinterpret_cast<uint32_t*>(tally));
    else
        hipLaunchKernelGGL(k_grid_tally, dim3((g.n + 255u) / 256u), dim3(256), 0, static_cast<hipStream_t>(stream_), g, tables, cells, occl,
                           reinterpret_cast<uint32_t*>(tally));
    return (int)hipGetLastError();
}

// out[i] = the ordered sum of surfel i < n over its `samples` items, in item order or (`linear`) in linear order
int launch_direct_fold(const uint8_t* occl, const float* contrib, uint32_t n, uint32_t samples, uint32_t linear, rb_radiance* out, void* stream_) {
    if (n == 0u) return 0;
    if (occl == nullptr || contrib == nullptr || out == nullptr || samples == 0u) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_direct_fold, dim3((n + 255u) / 256u), dim3(256), 0, static_cast<hipStream_t>(stream_), occl, contrib, n, samples, linear, out);
    return (int)hipGetLastError();
}

}  // namespace rb
