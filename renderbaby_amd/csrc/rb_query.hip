// rb_query.hip -- closest-hit queries (rb_cast_rays / rb_render_hits / rb_pick): the closest-hit search
// of one bounce-loop iteration (shader.wgsl:534-601) for a GIVEN ray, with the winner written out as an rb_hit and an
// rb_surface instead of being shaded.  Same numerics contract as rb_kernels.hip (no FMA contraction, correctly rounded / and
// sqrt), the same device functions for every test, and the walk a render of the scene would take:
//   k_query        trees of at most one node and at most 64 spheres: the scans
//   k_query_bvh    the per-lane reference walk (intersect_bvh) and, inside it, the per-lane sphere tree walk
//   k_query_chunk  the chunked walk: k_trace_chunk's node and pooled leaf phases, then the same finish per lane
// and their any-hit forms k_occl / k_occl_bvh / k_occl_chunk (rb_occluded) at the end of the file.
// One ray per lane on a plain grid sized to the piece.  Measured against a depth-1 render of the same frame -- the persistent
// grid with its item queue -- this form issues 15 % fewer vector instructions at a higher lane utilisation and, with pieces of
// 2^22 rays, takes 14-17 % less time on the mesh scenes (profiles/r06_query_rate.txt); what did cost time was many small launches.
//
// Records leave through the wave's LDS corner: a lane's record is three 16-byte quads 48 bytes apart from its neighbour's, so
// direct stores would touch every 64-byte sector of the wave's 3 KiB three times with a quarter of it each.  Staged, a wave
// writes its 64 records as three stores of 64 consecutive quads (ray source) or as eight runs of 384 bytes (pixel source: one
// run per row of its 8x8 tile) -- whole sectors -- and the device buffer is already in the ABI's layout: the read-back is one
// copy, into page-locked caller memory a DMA with no host pass.  (Three planes of quads would coalesce as well but leave the
// interleaving to the host.)
#include "rb_device_chunk.hpp"
#include "rb_device_centre.hpp"

#pragma clang fp contract(off)

namespace rb {
namespace {

#ifndef RB_QUERY_BLOCK
#define RB_QUERY_BLOCK 64
#endif
// threads per block (64, 128 or 256).  One wave per block: a block gives its LDS and its slot back when its wave's slowest ray is
// done, not when the slowest of four waves is (lamp fixture 1.22 -> 1.17 ms, C5 1.68 -> 1.62 ms; profiles/r06_query_rate.txt)
constexpr uint32_t kQueryBlock = RB_QUERY_BLOCK;
static_assert(kQueryBlock == 64 || kQueryBlock == 128 || kQueryBlock == 256, "whole waves, at most the stacks' 256 columns");
constexpr uint32_t kQueryWaveLds = 64u * 48u;   // one wave's 64 records of 48 B
static_assert(kQueryWaveLds == kChunkWaveLds, "k_query_chunk stages its records in the corner its walk has finished with");

// This lane's ray and where its record goes.
struct QueryLane {
    f3 o, d;
    bool live;    // there is a ray (ray source: index < n; pixel source: inside the window)
    bool valid;   // ... and it is finite after normalisation, and for a pixel inside the image
};

// a direction the walks can take: finite and not zero (a vector whose squared length overflows normalises to (0, 0, 0): every
// slab test would say "enter", and |d| = 1 +- 4 ulp, what the culling margins are derived for, would not hold)
DEV bool usable_dir(f3 d) { return finite3(d) && !(d.x == 0.0f && d.y == 0.0f && d.z == 0.0f); }

// `wave`: the wave's index in the launch.  Ray source: rays wave * 64 + lane.  Pixel source: tile `wave` of the window,
// 8 x 8 pixels in DISPLAYED coordinates (x mirrored: shader x = width - 1 - displayed x).
DEV QueryLane query_lane(const KParams& p, const QueryArgs q, uint32_t wave, uint32_t lane) {
    QueryLane r;
    r.o = r.d = mk(0, 0, 0);
    if (q.rays != nullptr) {
        const uint32_t i = wave * 64u + lane;
        r.live = i < q.n;
        if (r.live) {
            const v4f a = ((const v4f*)q.rays)[(size_t)i * 2u], b = ((const v4f*)q.rays)[(size_t)i * 2u + 1u];
            r.o = mk(a.x, a.y, a.z);
            r.d = normalize(mk(b.x, b.y, b.z));
        }
        r.valid = r.live && finite3(r.o) && usable_dir(r.d);
        return r;
    }
    const uint32_t tiles_x = (q.win_w + 7u) / 8u;
    const uint32_t tx = wave % tiles_x, ty = wave / tiles_x;
    const uint32_t cx = tx * 8u + (lane & 7u), cy = ty * 8u + (lane >> 3);
    r.live = cx < q.win_w && cy < q.win_h;
    const uint32_t xd = q.win_x + cx, row = q.win_y + cy;
    const uint32_t y = q.win_global ? row : global_row(p, row);
    r.valid = r.live && xd < p.u.width && y < p.u.height;
    if (r.valid) {
        r.o = ld3(p.cam.pos);
        r.d = centre_ray_dir(p.cam, p.u.width - 1u - xd, y);
        r.valid = finite3(r.o) && usable_dir(r.d);
    }
    return r;
}

// The wave's 64 records (three quads per lane) through `stage` (64 * 48 B of LDS) to `dst` in the ABI's layout.
DEV void store_records(const QueryArgs q, uint32_t wave, uint32_t lane, lds_v4f* stage, v4f rec0, v4f rec1, v4f rec2, void* dst_) {
    v4f* const dst = (v4f*)dst_;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();   // whoever read this corner before is done with it
    stage[lane * 3u] = rec0;
    stage[lane * 3u + 1u] = rec1;
    stage[lane * 3u + 2u] = rec2;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (uint32_t k = 0; k < 3u; k++) {
        const uint32_t j = k * 64u + lane;   // quad j of the wave = quad j % 3 of its record j / 3
        const v4f val = stage[j];
        if (q.rays != nullptr) {
            const uint32_t first = wave * 64u;   // (the last block's spare waves start beyond n: they store nothing)
            const uint32_t n = first >= q.n ? 0u : q.n - first < 64u ? q.n - first : 64u;
            if (j < n * 3u) dst[(size_t)first * 3u + j] = val;
        } else {
            const uint32_t tiles_x = (q.win_w + 7u) / 8u;   // (>= 1: the pixel source has no empty window)
            const uint32_t tx = wave % tiles_x, ty = wave / tiles_x;
            const uint32_t r = j / 24u, w = j % 24u;   // row of the tile, quad within the row's 8 records
            const uint32_t cy = ty * 8u + r, cx = tx * 8u + w / 3u;
            if (cy < q.win_h && cx < q.win_w) dst[((size_t)cy * q.win_w + tx * 8u) * 3u + w] = val;
        }
    }
}

// everything after the triangle walk: ground, spheres, lights, the winner's record, the stores
DEV void query_finish(const KParams& p, const QueryArgs q, const QueryLane& ql, const TriHit th, uint32_t* stack, uint32_t stride,
                      uint32_t wave, uint32_t lane, lds_v4f* stage) {
    HitQuads out;
    hit_quads_empty(out, 0xFFFFFFFFu /* RB_HIT_INVALID */, mk(0, 0, 0));
    if (ql.valid) {
        Tally<false> tl;
        Path pt;
        pt.o = ql.o;
        pt.d = ql.d;
        const SegState st = segment_pre<false>(fresh_params(p), pt, th, tl);
        float closest_t = st.closest_t;
        uint32_t sphere_idx = 0xFFFFFFFFu;
        segment_spheres<false, true>(fresh_params(p), ql.o, ql.d, dot(ql.d, ql.d), closest_t, sphere_idx, stack, stride, tl);
        segment_resolve(fresh_params(p), ql.o, ql.d, th, st, closest_t, sphere_idx, out);
    }
    store_records(q, wave, lane, stage, out.h0, out.h1, out.h2, q.hits);
    if (q.surf != nullptr) store_records(q, wave, lane, stage, out.s0, out.s1, out.s2, q.surf);
}

// ---- the per-lane walks.  MULTI = false: trees of at most one node (the multi-node walk stays out of the kernel).
template <bool MULTI>
__global__ void __launch_bounds__(kQueryBlock) k_query(const KParams p, const QueryArgs q) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_stack[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = blockIdx.x * (kQueryBlock / 64u) + (tid >> 6);
    uint32_t* const stack = stack_column(s_stack, tid);
    lds_v4f* const stage = (lds_v4f*)(reinterpret_cast<unsigned char*>(s_stack + p.stack_depth * kQueryBlock) + (tid >> 6) * kQueryWaveLds);
    const QueryLane ql = query_lane(fresh_params(p), q, wave, lane);
    TriHit th;
    th.hit = false;
    th.t = 1e20f;
    th.u = th.v = 0.0f;
    th.slot = 0u;
    if (ql.valid) {
        Tally<false> tl;
        th = intersect_bvh<false, MULTI>(fresh_params(p), ql.o, ql.d, stack, kQueryBlock, tl);
    }
    query_finish(p, q, ql, th, stack, kQueryBlock, wave, lane, stage);
}

// ---- the chunked walk (rb_device_chunk.hpp) with nothing to refill: a lane leaves the loop's work when its walk is complete, the
// wave when all have.
__global__ void __launch_bounds__(kQueryBlock) k_query_chunk(const KParams p, const QueryArgs q) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_stack[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = blockIdx.x * (kQueryBlock / 64u) + (tid >> 6);
    uint32_t* const stack = stack_column(s_stack, tid);
    const ChunkLds wl = chunk_lds(s_stack, p.stack_depth, kQueryBlock, tid);
    Tally<false> tl;

    const QueryLane ql = query_lane(fresh_params(p), q, wave, lane);
    const f3 o = ql.o, d = ql.d;
    ChunkLane L = {kChunkNone, kChunkNone, 0, kChunkNoHit, kChunkDone};
    const f3 inv = mk(rcp_exact(d.x), rcp_exact(d.y), rcp_exact(d.z));
    if (ql.valid) L = chunk_begin<false>(fresh_params(p), o, inv, L, tl);
    chunk_set_aside(L, stack, kQueryBlock);   // (a root that is one chunk)

    while (__ballot(L.state == kChunkWalk) != 0ull) {
        L = chunk_node_phase<false>(p, stack, kQueryBlock, o, d, inv, __uint_as_float((uint32_t)(L.key >> 32)), L, tl);
        chunk_leaf_phase<false, true, false>(p, wl, lane, o, d, L, tl, [&L, &wl, lane, stack](bool lf) {
            L.key = wl.best[lane];
            L = chunk_leaf_retire(L, lf, stack, kQueryBlock);
        });
    }
    query_finish(p, q, ql, chunk_winner(fresh_params(p), o, d, L.key), stack, kQueryBlock, wave, lane, wl.rayrec);
}

// ================================================================= any-hit occlusion ====
// out[i] = is there a hit with 0.001 < t < tmax[i] in the stages of `mask`?  The closest-hit search with its running bound fixed
// at tmax: every test is the same device function on the same operands, a lane leaves at the first one that accepts.  The
// stages run cheapest first -- ground, lights, spheres, triangles -- which an existential answer allows.
constexpr uint32_t kOcclVisible = RB_OCCL_VISIBLE, kOcclOccluded = RB_OCCL_OCCLUDED, kOcclInvalid = RB_OCCL_INVALID;

struct OcclLane {
    QueryLane ql;
    float tmax;     // min(tmax[i], 1e20f)
    uint32_t res;   // the byte so far: INVALID, or VISIBLE
    bool walk;      // valid, a bound above 0.001 and a stage to ask
};

DEV OcclLane occl_lane(const KParams& p, const OcclArgs& a, uint32_t wave, uint32_t lane) {
    OcclLane r;
    r.ql = query_lane(p, a.q, wave, lane);
    r.tmax = 1e20f;
    r.res = kOcclInvalid;
    r.walk = false;
    if (r.ql.live) {
        const float tm = a.tmax != nullptr ? a.tmax[(size_t)wave * 64u + lane] : 1e20f;
        if (r.ql.valid && tm == tm) {
            r.res = kOcclVisible;
            r.tmax = fminf(tm, 1e20f);
            r.walk = r.tmax > 0.001f && a.mask != 0u;
        }
    }
    return r;
}

// one result byte per lane: a wave's 64 consecutive bytes
DEV void occl_store(const OcclArgs& a, const OcclLane& ol, uint32_t wave, uint32_t lane, bool occluded) {
    if (ol.ql.live) a.out[(size_t)wave * 64u + lane] = (uint8_t)(occluded ? kOcclOccluded : ol.res);
}

// segment_spheres' / segment_resolve's scan of 96-byte {centre, radius | material} records with the bound fixed at tmax
DEV bool occl_scan(cf4p rec, uint32_t count, f3 o, f3 d, float a, float tmax) {
    for (uint32_t base = 0; base < count; base += 32u) {
        const uint32_t n = (count - base < 32u) ? count - base : 32u;
        uint32_t cand = 0u;
        for (uint32_t k = 0; k < n; k++) {
            const v4f cr = rec[(size_t)(base + k) * 6u];
            const f3 oc = o - mk(cr.x, cr.y, cr.z);
            const float half_b = dot(oc, d);
            const float c = dot(oc, oc) - cr.w * cr.w;
            const float disc = half_b * half_b - a * c;
            cand |= (disc < 0.0f) ? 0u : (1u << k);
        }
        while (cand != 0u) {
            const uint32_t k = (uint32_t)__ffs((int)cand) - 1u;
            cand &= cand - 1u;
            const v4f cr = rec[(size_t)(base + k) * 6u];
            const float t = isect_sphere(o, d, a, mk(cr.x, cr.y, cr.z), cr.w);
            if (t > 0.001f && t < tmax) return true;
        }
    }
    return false;
}

// intersect_spheres_bvh with the bound fixed at tmax: sphere_child's cull `tn - dt > best` is argued for any best that bounds
// the reported t of a hit that matters, and every hit that matters here is below tmax
DEV bool occl_spheres_bvh(const KParams& p, f3 o, f3 d, float a, float tmax, uint32_t* stack, uint32_t stride) {
    const f3 inv = mk(__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y), __builtin_amdgcn_rcpf(d.z));
    const uint32_t dneg = sph_dir_signs(d);
    const cf4p leafs = (cf4p)p.sph_leaf;
    uint32_t cur = p.sph_root;
    int sp = 0;
    for (;;) {
        if (cur != kSphNone && (cur & 0x80000000u) == 0u) {
            cur = sphere_node_step(p, cur, o, inv, dneg, tmax, [&](uint32_t ref) {
                stack[sp * stride] = ref;
                sp++;
            });
            if (cur != kSphNone) continue;
        } else if (cur != kSphNone) {
            const uint32_t first = sph_leaf_first(cur), count = sph_leaf_count(cur);
            for (uint32_t j = first; j < first + count; j++) {
                const v4f cr = leafs[j];
                const float t = isect_sphere(o, d, a, mk(cr.x, cr.y, cr.z), cr.w);
                if (t > 0.001f && t < tmax) return true;
            }
        }
        if (sp == 0) return false;
        sp--;
        cur = stack[sp * stride];
    }
}

// ground, lights, spheres (shader.wgsl:552-565, :590-601, :574-586)
template <bool SPHTREE>
DEV bool occl_early(const KParams& p, uint32_t mask, f3 o, f3 d, float tmax, uint32_t* stack, uint32_t stride) {
    if ((mask & RB_MASK_GROUND) != 0u && p.u.ground_enabled > 0u) {
        const float t = isect_ground(o, d, p.u.ground_height);
        if (t > 0.001f && t < tmax) return true;
    }
    const float a = dot(d, d);
    if ((mask & RB_MASK_LIGHTS) != 0u && occl_scan((cf4p)p.lights, p.n_lights, o, d, a, tmax)) return true;
    if ((mask & RB_MASK_SPHERES) != 0u) {
        if constexpr (SPHTREE) {
            if (p.sph_nodes != nullptr) return occl_spheres_bvh(p, o, d, a, tmax, stack, stride);
        }
        return occl_scan((cf4p)p.spheres, p.u.spheres_count, o, d, a, tmax);
    }
    return false;
}

// intersect_bvh's reference walk (never the library's own tree: query_walk clears fast_nodes for every query): the
// same nodes entered by the same boolean box tests, the same triangles tested, test_slot's acceptance against tmax
template <bool MULTI>
DEV bool occl_bvh(const KParams& p, f3 o, f3 d, float tmax, uint32_t* stack, uint32_t stride) {
    const uint32_t node_count = p.u.bvh_node_count;
    if (node_count == 0u) return false;
    const f3 inv = mk(rcp_exact(d.x), rcp_exact(d.y), rcp_exact(d.z));
    const cf4p nodes = (cf4p)p.nodes;
    const cf4p ptris = (cf4p)p.ptris;
    float u, v;
    if (node_count == 1u) {
        const v4f n0 = nodes[0], n1 = nodes[1];
        const v4u n2 = ((cu4p)p.nodes)[2];
        const uint32_t first = n2.z, count = n2.w;
        const uint32_t end = (first + count < p.index_len) ? first + count : p.index_len;  // guard :331
        if (first < end && isect_aabb(o, inv, mk(n0.x, n0.y, n0.z), mk(n1.x, n1.y, n1.z))) {
            for (uint32_t slot = first; slot < end; slot++) {
                const v4f a = ptris[(size_t)slot * 4u], b = ptris[(size_t)slot * 4u + 1u], c = ptris[(size_t)slot * 4u + 2u];
                if (__float_as_uint(c.w) == 0u) continue;  // guard :336
                const float t = isect_triangle(o, d, mk(a.x, a.y, a.z), mk(b.x, b.y, b.z), mk(c.x, c.y, c.z), u, v);
                if (t > 0.001f && t < tmax) return true;
            }
        }
        return false;
    }
    if constexpr (!MULTI) return false;
    int sp = 1;
    stack[0] = 0u;
    while (sp > 0) {
        sp--;
        const uint32_t node_idx = stack[sp * stride];
        if (node_idx >= node_count) continue;
        const v4f n0 = nodes[node_idx * 3u], n1 = nodes[node_idx * 3u + 1u];
        const v4u n2 = ((cu4p)p.nodes)[node_idx * 3u + 2u];
        if (!isect_aabb(o, inv, mk(n0.x, n0.y, n0.z), mk(n1.x, n1.y, n1.z))) continue;
        const uint32_t left = n2.x, right = n2.y, first = n2.z, count = n2.w;
        if (count > 0u) {
            for (uint32_t i = 0; i < count; i++) {
                const uint32_t slot = first + i;
                if (slot >= p.index_len) continue;
                const v4f a = ptris[slot * 4u], b = ptris[slot * 4u + 1u], c = ptris[slot * 4u + 2u];
                if (__float_as_uint(c.w) == 0u) continue;  // guard :336
                const float t = isect_triangle(o, d, mk(a.x, a.y, a.z), mk(b.x, b.y, b.z), mk(c.x, c.y, c.z), u, v);
                if (t > 0.001f && t < tmax) return true;
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
    return false;
}

// ---- the per-lane walks.  MULTI = false: trees of at most one node and at most 64 spheres, no stack.
template <bool MULTI>
__global__ void __launch_bounds__(kQueryBlock) k_occl(const KParams p, const OcclArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_stack[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = blockIdx.x * (kQueryBlock / 64u) + (tid >> 6);
    uint32_t* const stack = stack_column(s_stack, tid);
    const OcclLane ol = occl_lane(fresh_params(p), a, wave, lane);
    bool occluded = false;
    if (ol.walk) {
        occluded = occl_early<MULTI>(fresh_params(p), a.mask, ol.ql.o, ol.ql.d, ol.tmax, stack, kQueryBlock);
        if (!occluded && (a.mask & RB_MASK_TRIANGLES) != 0u)
            occluded = occl_bvh<MULTI>(fresh_params(p), ol.ql.o, ol.ql.d, ol.tmax, stack, kQueryBlock);
    }
    occl_store(a, ol, wave, lane, occluded);
}

// ---- the chunked walk with every lane's entry of `best` starting each round at (bits(tmax) << 32) and the nodes culled on tmax
// with the section 4.2 margin from the first step: that margin bounds the reference's reported t of any accepted hit below a
// child, so no triangle with a reported t < tmax is culled.  The pooled lanes fold their t into best[ray] as in k_query_chunk; a
// ray whose best t has come below tmax after a round is answered and leaves the walk.
__global__ void __launch_bounds__(kQueryBlock) k_occl_chunk(const KParams p, const OcclArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_stack[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = blockIdx.x * (kQueryBlock / 64u) + (tid >> 6);
    uint32_t* const stack = stack_column(s_stack, tid);
    const ChunkLds wl = chunk_lds(s_stack, p.stack_depth, kQueryBlock, tid);
    Tally<false> tl;

    const OcclLane ol = occl_lane(fresh_params(p), a, wave, lane);
    const f3 o = ol.ql.o, d = ol.ql.d;
    bool occluded = false;
    if (ol.walk) occluded = occl_early<true>(fresh_params(p), a.mask, o, d, ol.tmax, stack, kQueryBlock);
    const uint32_t tmax_bits = __float_as_uint(ol.tmax);     // (positive: bit patterns order like the values)
    ChunkLane L = {kChunkNone, kChunkNone, 0, (unsigned long long)tmax_bits << 32, kChunkDone};
    const f3 inv = mk(rcp_exact(d.x), rcp_exact(d.y), rcp_exact(d.z));
    if (ol.walk && !occluded && (a.mask & RB_MASK_TRIANGLES) != 0u) L = chunk_begin<false>(fresh_params(p), o, inv, L, tl);
    chunk_set_aside(L, stack, kQueryBlock);   // (a root that is one chunk)

    while (__ballot(L.state == kChunkWalk) != 0ull) {
        L = chunk_node_phase<false>(p, stack, kQueryBlock, o, d, inv, ol.tmax, L, tl);
        chunk_leaf_phase<false, false, false>(p, wl, lane, o, d, L, tl, [&L, &wl, &occluded, lane, stack, tmax_bits](bool lf) {
            if ((uint32_t)(wl.best[lane] >> 32) < tmax_bits) {   // a reported t with 0.001 < t < tmax: answered
                occluded = true;
                L.state = kChunkDone;
                L.cur = kChunkNone;
                L.sp = 0;
            }
            L = chunk_leaf_retire(L, lf, stack, kQueryBlock);
        });
    }
    occl_store(a, ol, wave, lane, occluded);
}

}  // namespace

int launch_query(const KParams& p_, const QueryArgs& q, void* stream_, LaunchInfo* info) {
    KParams p = p_;
    p.cam = host_cam(p.u);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    LaunchInfo li{};
    li.block = kQueryBlock;
    const uint64_t waves = q.rays != nullptr ? ((uint64_t)q.n + 63u) / 64u : (uint64_t)((q.win_w + 7u) / 8u) * ((q.win_h + 7u) / 8u);
    if (waves == 0u || waves > 0x7FFFFFFFull) return waves == 0u ? 0 : (int)hipErrorInvalidValue;
    li.grid = (uint32_t)((waves + kQueryBlock / 64u - 1u) / (kQueryBlock / 64u));
    li.lds_bytes = (size_t)kStackEntryBytes * p.stack_depth * kQueryBlock + (kQueryBlock / 64u) * kQueryWaveLds;
    const dim3 grid(li.grid), block(li.block);
    switch (query_walk(p)) {
        case kWalkChunk:
            li.kernel_name = "k_query_chunk";
            hipLaunchKernelGGL(k_query_chunk, grid, block, li.lds_bytes, stream, p, q);
            break;
        case kWalkBvh:
            li.kernel_name = "k_query_bvh";
            hipLaunchKernelGGL(k_query<true>, grid, block, li.lds_bytes, stream, p, q);
            break;
        case kWalkPlain:
            li.kernel_name = "k_query";
            hipLaunchKernelGGL(k_query<false>, grid, block, li.lds_bytes, stream, p, q);
            break;
    }
    if (info) *info = li;
    return (int)hipGetLastError();
}

int launch_occluded(const KParams& p_, const OcclArgs& a, void* stream_, LaunchInfo* info) {
    KParams p = p_;
    p.cam = host_cam(p.u);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    LaunchInfo li{};
    li.block = kQueryBlock;
    const uint64_t waves = ((uint64_t)a.q.n + 63u) / 64u;
    if (a.q.rays == nullptr || a.out == nullptr || waves > 0x7FFFFFFFull) return (int)hipErrorInvalidValue;
    if (waves == 0u) return 0;
    li.grid = (uint32_t)((waves + kQueryBlock / 64u - 1u) / (kQueryBlock / 64u));
    li.lds_bytes = (size_t)kStackEntryBytes * p.stack_depth * kQueryBlock;
    const dim3 grid(li.grid), block(li.block);
    switch (query_walk(p)) {
        case kWalkChunk:
            li.kernel_name = "k_occl_chunk";
            li.lds_bytes += (kQueryBlock / 64u) * kChunkWaveLds;
            hipLaunchKernelGGL(k_occl_chunk, grid, block, li.lds_bytes, stream, p, a);
            break;
        case kWalkBvh:
            li.kernel_name = "k_occl_bvh";
            hipLaunchKernelGGL(k_occl<true>, grid, block, li.lds_bytes, stream, p, a);
            break;
        case kWalkPlain:
            li.kernel_name = "k_occl";
            hipLaunchKernelGGL(k_occl<false>, grid, block, li.lds_bytes, stream, p, a);
            break;
    }
    if (info) *info = li;
    return (int)hipGetLastError();
}

}  // namespace rb
