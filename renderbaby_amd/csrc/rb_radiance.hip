// rb_radiance.hip -- path-traced radiance along caller-given rays (rb_trace_rays): trace_ray
// (shader.wgsl:522-662) for a GIVEN ray and a seed made from the caller's id of the ray, summed over `samples` samples.
// Same numerics contract as rb_kernels.hip (no FMA contraction, correctly rounded / and sqrt), the same device functions
// for every test and for the shading, and the walk a render of the scene would take:
//   k_rad        trees of at most one node and at most 64 spheres: k_trace_direct's per-segment loop
//   k_rad_bvh    k_trace_bvh's stepped reference walk and, inside segment_finish, the per-lane sphere tree walk
//   k_rad_chunk  the chunked walk: k_trace_chunk's node and pooled leaf phases
// Like the render's stream kernels these are persistent wavefronts over a queue of (ray, sample) items with path
// regeneration -- a lane whose path ends takes the next item while its neighbours keep walking -- and like them they
// work in two phases ("Why two phases"): a finished path stores its colour (16 B) into a scratch
// laid out [block of 64 rays][sample][64 rays], and k_rad_sum, one lane per ray, adds a ray's samples IN SAMPLE ORDER.
// What differs from the render is where a path starts (two 16-byte loads of the ray, its normalisation, the seed; no
// camera, no jitter draws) and where its colour ends up (a per-ray sum instead of the frame's accumulation).  Only
// non-STATS forms exist: the work counters do not move.
// Each body is a template on where a path starts: k_rad* start on the caller's ray (RayStart), k_cam* on the record the camera
// generator made for the item (CamStart; rb_camera.hip) -- the same queue, walks and sum behind both.
#include "rb_device_chunk.hpp"
#include "rb_launch_plan.hpp"

#pragma clang fp contract(off)

namespace rb {
namespace {

constexpr uint32_t kRadBlock = 256;
#ifndef RB_RAD_WAVES
#define RB_RAD_WAVES 6         // k_trace's: 80 registers
#endif
#ifndef RB_RAD_BVH_WAVES
#define RB_RAD_BVH_WAVES 1     // k_trace_bvh's
#endif
#ifndef RB_RAD_CHUNK_WAVES
#define RB_RAD_CHUNK_WAVES 5   // k_trace_chunk's: 96 registers
#endif
#ifndef RB_RAD_FINISH_LANES
#define RB_RAD_FINISH_LANES 32 // k_trace_chunk's RB_CHUNK_FINISH_LANES
#endif

// ---- (ray, sample) items.  Item = (block * S + sample) * 64 + ray-in-block, block = 64 consecutive rays of the piece.
// A refill round hands out at most 64 consecutive items starting at the wave-uniform `base`, so a lane's item lies in the
// 64-item row of `base` or in the next one (item_rows' argument, rb_device_shade.hpp).
struct RadRows {
    uint32_t in0;
    uint32_t blk[2], hs[2];   // the row's block of rays and pcg(first_sample + its sample)
};
DEV RadRows rad_rows(const RadArgs& a, uint32_t base) {
    RadRows r;
    r.in0 = base & 63u;
    uint32_t smp;
    const uint32_t blk = udiv_magic(base >> 6, a.samples, a.magic_S, smp);
    r.blk[0] = blk;
    r.hs[0] = pcg(a.first_sample + smp);
    uint32_t smp1 = smp + 1u, blk1 = blk;
    if (smp1 == a.samples) {
        smp1 = 0u;
        blk1++;
    }
    r.blk[1] = blk1;
    r.hs[1] = pcg(a.first_sample + smp1);
    return r;
}

// The start of item `it`'s path on the calling lane: the ray as rb_cast_rays reads it (query_lane, rb_query.hip: two
// 16-byte loads, the device's normalize), seed(i, k) = pcg(sid_i + pcg(first_sample + k)) -- the first line of the
// shader's main with sid_i in place of pixel_index; no jitter draws follow.  False for a ray that is not walked: an invalid
// one (its colour slot becomes {0, 0, 0, 0}: weight 0) or any ray at max_depth = 0 ({0, 0, 0, 1}).
DEV bool rad_start(const KParams& p, const RadArgs& a, uint32_t it, uint32_t ray, uint32_t hs, Path& pt) {
    const v4f ra = ((const v4f*)a.rays)[(size_t)ray * 2u], rd = ((const v4f*)a.rays)[(size_t)ray * 2u + 1u];
    pt.o = mk(ra.x, ra.y, ra.z);
    pt.d = normalize(mk(rd.x, rd.y, rd.z));
    const bool valid = finite3(pt.o) && finite3(pt.d) && !(pt.d.x == 0.0f && pt.d.y == 0.0f && pt.d.z == 0.0f);
    const uint32_t sid = a.seeds != nullptr ? a.seeds[ray] : a.seed_base + ray;
    pt.seed = pcg(sid + hs);
    pt.color = mk(0, 0, 0);
    pt.att = mk(1, 1, 1);
    pt.depth = 0;
    if (valid && p.u.max_depth > 0u) return true;
    const v4f v = {0.0f, 0.0f, 0.0f, valid ? 1.0f : 0.0f};
    reinterpret_cast<v4f*>(a.colors)[it] = v;
    return false;
}

// Where a kernel's paths start.  RayStart: the caller's ray (rb_trace_rays).  CamStart: the item's own record as k_cam_rays
// (rb_camera.hip) left it in item order -- {o, seed bits}, {d, 0}: two 16-byte loads.  The generator has
// normalised d, drawn from the seed and zeroed the direction of an invalid ray, so nothing is normalised or hashed here.
struct RayStart {
    static DEV bool start(const KParams& p, const RadArgs& a, uint32_t it, uint32_t ray, uint32_t hs, Path& pt) {
        return rad_start(p, a, it, ray, hs, pt);
    }
};
struct CamStart {
    static DEV bool start(const KParams& p, const RadArgs& a, uint32_t it, uint32_t, uint32_t, Path& pt) {
        const v4f ra = ((const v4f*)a.rays)[(size_t)it * 2u], rd = ((const v4f*)a.rays)[(size_t)it * 2u + 1u];
        pt.o = mk(ra.x, ra.y, ra.z);
        pt.d = mk(rd.x, rd.y, rd.z);
        const bool valid = !(pt.d.x == 0.0f && pt.d.y == 0.0f && pt.d.z == 0.0f);
        pt.seed = __float_as_uint(ra.w);
        pt.color = mk(0, 0, 0);
        pt.att = mk(1, 1, 1);
        pt.depth = 0;
        if (valid && p.u.max_depth > 0u) return true;
        const v4f v = {0.0f, 0.0f, 0.0f, valid ? 1.0f : 0.0f};
        reinterpret_cast<v4f*>(a.colors)[it] = v;
        return false;
    }
};

// a finished path: its colour and weight 1 into its (ray, sample) slot, read once by k_rad_sum (a streaming store, as
// store_color of rb_kernels.hip)
DEV void rad_store(const RadArgs& a, uint32_t it, f3 c) {
    const v4f v = {c.x, c.y, c.z, 1.0f};
    __builtin_nontemporal_store(v, reinterpret_cast<v4f*>(a.colors) + it);
}

// The work queue, one instance per wavefront: ItemQueue of rb_kernels.hip with one queue word and no bands.  The first
// reservation is the wave's own -- wave w starts on items [w * batch, (w + 1) * batch) and the queue word starts at
// waves * batch (launch_radiance) --, later ones are one atomic per `batch` items; inside a reservation the wave hands
// items to its idle lanes with ballot + prefix count.
struct RadQueue {
    uint32_t loc_next = 0, loc_end = 0;   // this wave's reserved item range (wave-uniform)
    uint32_t batch, total;
    bool exhausted = false;

    DEV RadQueue(const RadArgs& a, uint32_t total_items) : batch(a.batch), total(total_items) {
        const uint64_t first = (uint64_t)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * batch;
        if (first < total) {
            loc_next = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)first);
            loc_end = (total - loc_next < batch) ? total : loc_next + batch;
        }
    }
    DEV bool drained() const { return exhausted && loc_next == loc_end; }

    // on_item(item, ray, sample_hash) starts a path on the calling lane; the padding rays of the last block are skipped here
    template <class IsIdle, class OnItem>
    DEV void refill(const RadArgs& a, uint32_t lane, IsIdle&& is_idle, OnItem&& on_item) {
        unsigned long long idle = __ballot(is_idle());
        for (int round = 0; round < 2 && idle != 0ull; round++) {
            if (loc_next == loc_end) {
                if (exhausted) break;
                uint32_t b = 0;
                if (lane == 0u) b = atomicAdd(a.queue, batch);
                b = (uint32_t)__builtin_amdgcn_readfirstlane((int)b);
                if (b >= total) {
                    exhausted = true;
                    break;
                }
                loc_next = b;
                loc_end = (total - b < batch) ? total : b + batch;
            }
            const RadRows rows = rad_rows(a, loc_next);
            const uint32_t avail = loc_end - loc_next;
            const uint32_t rank = (uint32_t)__popcll(idle & ((1ull << lane) - 1ull));
            const bool take = ((idle >> lane) & 1ull) != 0ull && rank < avail;
            const uint32_t n_idle = (uint32_t)__popcll(idle);
            const uint32_t taken = n_idle < avail ? n_idle : avail;
            if (take) {
                const uint32_t idx = rows.in0 + rank;
                const bool next = idx >= 64u;
                const uint32_t ray = (next ? rows.blk[1] : rows.blk[0]) * 64u + (idx & 63u);
                if (ray < a.n) on_item(loc_next + rank, ray, next ? rows.hs[1] : rows.hs[0]);
            }
            loc_next += taken;
            idle = __ballot(is_idle());
            if (taken == n_idle) break;   // everyone who asked was served (or got a padding item)
        }
    }
};

DEV uint32_t rad_total_items(const RadArgs& a) { return ((a.n + 63u) / 64u) * a.samples * 64u; }   // host keeps this < 2^31

// ============================================================== k_rad ====
// k_trace_direct's loop (rb_kernels.hip, trace_body<.., MULTI = false, STAGED = false>): every lane starts its own path
// when it is handed the item and stores its colour directly; no ColorRing staging.
template <class Start>
DEV void rad_body(const KParams& p, const RadArgs& a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_stack[];
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u;
    Tally<false> tl;
    bool active = false;
    uint32_t item = 0;
    RadQueue iq(a, rad_total_items(a));
    Path pt;
    pt.depth = 0;

    for (;;) {
        iq.refill(a, lane, [&] { return !active; },
                  [&](uint32_t it, uint32_t ray, uint32_t hs) {
                      item = it;
                      active = Start::start(fresh_params(p), a, it, ray, hs, pt);
                  });
        if (__ballot(active) == 0ull) {
            if (iq.drained()) break;
            continue;
        }
        if (active) {
            const bool alive = segment<false, false>(p, pt, &s_stack[tid], kRadBlock, tl);
            if (!alive) {
                rad_store(a, item, pt.color);
                active = false;
            }
        }
    }
}
__global__ void __launch_bounds__(kRadBlock, RB_RAD_WAVES) k_rad(const KParams p, const RadArgs a) { rad_body<RayStart>(p, a); }
__global__ void __launch_bounds__(kRadBlock, RB_RAD_WAVES) k_cam(const KParams p, const RadArgs a) { rad_body<CamStart>(p, a); }

// ========================================================== k_rad_bvh ====
// k_trace_bvh's stepped reference walk (rb_kernels.hip; the form that reads the tree through L1 / L2): the scheduling unit
// is one leaf, the visit order per ray is the reference's, so the winner is the same triangle.  segment_finish carries the
// per-lane sphere tree walk for scenes with more than 64 spheres.
template <class Start>
DEV void rad_bvh_body(const KParams& p, const RadArgs& a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_stack[];
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u;
    const uint32_t node_count = p.u.bvh_node_count;
    const cf4p nodes = (cf4p)p.nodes;
    const cf4p ptris = (cf4p)p.ptris;
    uint32_t* const stack = stack_column(s_stack, tid);
    Tally<false> tl;

    enum : uint32_t { IDLE = 0, BEGIN = 1, TRAV = 2, FINISH = 3 };
    uint32_t state = IDLE;
    uint32_t item = 0;
    RadQueue iq(a, rad_total_items(a));
    Path pt;
    pt.depth = 0;
    TriHit th;
    th.hit = false;
    th.t = 1e20f;
    th.u = th.v = 0.0f;
    th.slot = 0u;
    f3 inv = mk(0, 0, 0);
    int sp = 0;

    for (;;) {
        // ---- (1) hand items to idle lanes
        iq.refill(a, lane, [&] { return state == IDLE; },
                  [&](uint32_t it, uint32_t ray, uint32_t hs) {
                      item = it;
                      if (Start::start(fresh_params(p), a, it, ray, hs, pt)) state = BEGIN;
                  });
        if (__ballot(state != IDLE) == 0ull) {
            if (iq.drained()) break;
            continue;
        }

        // ---- (2) start of a segment: reset the traversal (shader.wgsl:283-307)
        if (state == BEGIN) {
            th.hit = false;
            th.t = 1e20f;
            th.u = th.v = 0.0f;
            th.slot = 0u;
            inv = mk(rcp_exact(pt.d.x), rcp_exact(pt.d.y), rcp_exact(pt.d.z));
            stack[0] = 0u;
            sp = 1;
            state = TRAV;
        }

        // ---- (3) node phase: pop until this lane has a leaf to test or its stack is empty
        uint32_t first = 0, count = 0;
        while (state == TRAV && count == 0u) {
            if (sp == 0) {
                state = FINISH;
                break;
            }
            sp--;
            const uint32_t node_idx = stack[sp * kRadBlock];
            if (node_idx >= node_count) continue;
            const v4f n0 = nodes[node_idx * 3u], n1 = nodes[node_idx * 3u + 1u], n2f = nodes[node_idx * 3u + 2u];
            const uint32_t n_left = __float_as_uint(n2f.x), n_right = __float_as_uint(n2f.y),
                           n_first = __float_as_uint(n2f.z), n_count = __float_as_uint(n2f.w);
            if (!isect_aabb(pt.o, inv, mk(n0.x, n0.y, n0.z), mk(n1.x, n1.y, n1.z))) continue;
            if (n_count > 0u) {
                first = n_first;
                count = n_count;
            } else {
                if (n_left < node_count) {
                    stack[sp * kRadBlock] = n_left;
                    sp++;
                }
                if (n_right < node_count) {
                    stack[sp * kRadBlock] = n_right;
                    sp++;
                }
            }
        }

        // ---- (4) leaf phase: this lane's leaf (shader.wgsl:327-374); candidates are offered in slot order
        {
            const uint32_t end = (first + count < p.index_len) ? first + count : p.index_len;  // guard :331
            for (uint32_t slot = first; slot < end; slot++) {
                const v4f ta = ptris[slot * 4u], tb = ptris[slot * 4u + 1u], tc = ptris[slot * 4u + 2u];
                if (__float_as_uint(tc.w) == 0u) continue;  // guard :336
                test_slot(ta, tb, tc, slot, pt.o, pt.d, th);
            }
        }

        // ---- (5) traversal complete: ground, spheres, lights, shading, next ray
        if (state == FINISH) {
            const bool alive = segment_finish<false>(p, pt, th, stack, kRadBlock, tl);
            if (alive) {
                state = BEGIN;
            } else {
                rad_store(a, item, pt.color);
                state = IDLE;
            }
        }
    }
}
__global__ void __launch_bounds__(kRadBlock, RB_RAD_BVH_WAVES) k_rad_bvh(const KParams p, const RadArgs a) { rad_bvh_body<RayStart>(p, a); }
__global__ void __launch_bounds__(kRadBlock, RB_RAD_BVH_WAVES) k_cam_bvh(const KParams p, const RadArgs a) { rad_bvh_body<CamStart>(p, a); }

// ======================================================== k_rad_chunk ====
// The chunked walk (rb_device_chunk.hpp) over the rays of a buffer, scheduled like k_trace_chunk.
// SPHTREE: the instantiation for scenes that also have a sphere tree.
template <bool SPHTREE, class Start>
DEV void rad_chunk_body(const KParams& p, const RadArgs& a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_stack[];
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u;
    uint32_t* const stack = stack_column(s_stack, tid);
    Tally<false> tl;
    const ChunkLds wl = chunk_lds(s_stack, p.stack_depth, kRadBlock, tid);

    enum : uint32_t { IDLE = 0, BEGIN = 1, TRAV = kChunkWalk, FINISH = kChunkDone };   // L.state: the kernel's own two and the walk's two
    static_assert(IDLE != TRAV && IDLE != FINISH && BEGIN != TRAV && BEGIN != FINISH, "a lane that is idle or about to begin must not look like one that walks or is done");
    uint32_t item = 0;
    ChunkLane L = {0u, kChunkNone, 0, kChunkNoHit, IDLE};
    RadQueue iq(a, rad_total_items(a));
    Path pt;
    pt.depth = 0;
    f3 inv = mk(0, 0, 0);

    for (;;) {
        // ---- (1) hand items to idle lanes
        iq.refill(a, lane, [&] { return L.state == IDLE; },
                  [&](uint32_t it, uint32_t ray, uint32_t hs) {
                      item = it;
                      if (Start::start(fresh_params(p), a, it, ray, hs, pt)) L.state = BEGIN;
                  });
        if (__ballot(L.state != IDLE) == 0ull) {
            if (iq.drained()) break;
            continue;
        }

        // ---- (2) start of a segment
        if (L.state == BEGIN) {
            inv = mk(rcp_exact(pt.d.x), rcp_exact(pt.d.y), rcp_exact(pt.d.z));
            L.key = kChunkNoHit;
            L.sp = 0;
            L = chunk_begin<false>(fresh_params(p), pt.o, inv, L, tl);
        }

        // ---- (3) tree, (4) leaves: the walk's phases
        {
            L = chunk_node_phase<false>(p, stack, kRadBlock, pt.o, pt.d, inv, __uint_as_float((uint32_t)(L.key >> 32)), L, tl);
            chunk_leaf_phase<true, true, false>(p, wl, lane, pt.o, pt.d, L, tl, [&](bool lf) {
                L.key = wl.best[lane];
                L = chunk_leaf_retire(L, lf, stack, kRadBlock);
            });
        }

        // ---- (5) finished walks: the winner's record, the rest of the segment (shading), next ray
        {
            const uint32_t n_fin = (uint32_t)__popcll(__ballot(L.state == FINISH));
            const uint32_t n_trav = (uint32_t)__popcll(__ballot(L.state == TRAV));
            if (n_fin != 0u && (n_fin >= (uint32_t)RB_RAD_FINISH_LANES || n_trav == 0u) && L.state == FINISH) {
                const TriHit th = chunk_winner(fresh_params(p), pt.o, pt.d, L.key);
                const bool alive = segment_finish<false, SPHTREE>(p, pt, th, stack, kRadBlock, tl);
                if (alive) {
                    L.state = BEGIN;
                } else {
                    rad_store(a, item, pt.color);
                    L.state = IDLE;
                }
            }
        }
    }
}
template <bool SPHTREE>
__global__ void __launch_bounds__(kRadBlock, RB_RAD_CHUNK_WAVES) k_rad_chunk(const KParams p, const RadArgs a) {
    rad_chunk_body<SPHTREE, RayStart>(p, a);
}
template <bool SPHTREE>
__global__ void __launch_bounds__(kRadBlock, RB_RAD_CHUNK_WAVES) k_cam_chunk(const KParams p, const RadArgs a) {
    rad_chunk_body<SPHTREE, CamStart>(p, a);
}

// ========================================================== k_rad_sum ====
// Phase 2, shaped like k_accumulate: one wavefront per block of 64 rays, lane = ray; each sample row is a contiguous 1 KiB
// read.  The sum starts at +0 and adds the samples in ascending order, one binary32 add per component; the weights (1 per
// sample of a valid ray, 0 of an invalid one) add up to (float)samples or 0 exactly (samples <= 65536).
__global__ void __launch_bounds__(256) k_rad_sum(const RadArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t blk = blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t ray = blk * 64u + lane;
    if (ray >= a.n) return;
    const uint32_t S = a.samples;
    const nt_f4* __restrict__ c = reinterpret_cast<const nt_f4*>(a.colors) + ((size_t)blk * S) * 64u + lane;
    f3 acc = mk(0, 0, 0);
    float w = 0.0f;
    uint32_t s = 0;
    for (; s + 8u <= S; s += 8u) {
        nt_f4 v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = __builtin_nontemporal_load(&c[(size_t)(s + k) * 64u]);
#pragma unroll
        for (int k = 0; k < 8; k++) {
            acc = acc + mk(v[k].x, v[k].y, v[k].z);
            w = w + v[k].w;
        }
    }
    for (; s < S; s++) {
        const nt_f4 v = __builtin_nontemporal_load(&c[(size_t)s * 64u]);
        acc = acc + mk(v.x, v.y, v.z);
        w = w + v.w;
    }
    const v4f r = {acc.x, acc.y, acc.z, w};
    reinterpret_cast<v4f*>(a.out)[ray] = r;
}

}  // namespace

// One piece: a.n rays x a.samples samples, at most RB_TRACE_PIECE_ITEMS items (the caller cuts; a.colors holds them all).
// Queue word, trace kernel and sum are queued on `stream`; nothing is waited for.  `records`: a.rays holds one record per ITEM,
// in item order, as k_cam_rays writes them (rb_camera.hip) -- the k_cam kernels; a.seeds and a.seed_base are not read.
int launch_radiance(const KParams& p_, const RadArgs& a_, void* stream_, LaunchInfo* info, bool records) {
    KParams p = p_;
    p.cam = host_cam(p.u);
    RadArgs a = a_;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    LaunchInfo li{};
    li.block = kRadBlock;
    if (a.n == 0u) return 0;
    const uint64_t blocks64 = ((uint64_t)a.n + 63u) / 64u;
    const uint64_t items = blocks64 * 64u * a.samples;
    if (a.rays == nullptr || a.out == nullptr || a.colors == nullptr || a.queue == nullptr || a.samples == 0u || items > RB_TRACE_PIECE_ITEMS)
        return (int)hipErrorInvalidValue;
    const QueryWalk v = query_walk(p);
    static const char* const names[2][3] = {{"k_rad", "k_rad_bvh", "k_rad_chunk"}, {"k_cam", "k_cam_bvh", "k_cam_chunk"}};
    li.kernel_name = names[records ? 1 : 0][v];
    li.lds_bytes = (size_t)kStackEntryBytes * p.stack_depth * kRadBlock + (v == kWalkChunk ? (kRadBlock / 64u) * kChunkWaveLds : 0u);
    // grid and reservations by the trace launch's rules (rb_launch_plan.hpp): residency by registers, fewer blocks for a launch of few items
    const uint32_t cus = device_cu_count_cached();
    const uint32_t blocks_per_cu = p.blocks_per_cu ? p.blocks_per_cu : v == kWalkChunk ? (uint32_t)RB_RAD_CHUNK_WAVES : dense_blocks_per_cu(items, cus);
    li.grid = persistent_blocks(items, kRadBlock, cus, blocks_per_cu);
    const uint64_t waves = (uint64_t)li.grid * (kRadBlock / 64u);
    a.batch = p.queue_batch ? p.queue_batch : (uint32_t)reservation(items, waves, v == kWalkPlain);
    a.magic_S = magic_of(a.samples);
    // the queue starts behind the waves' own first reservations
    hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(a.queue), (int)(uint32_t)(waves * a.batch), 1, stream);
    if (e != hipSuccess) return (int)e;
    const dim3 g(li.grid), b(li.block);
    const bool sph = p.sph_nodes != nullptr;
    switch (v) {
        case kWalkPlain: hipLaunchKernelGGL(records ? k_cam : k_rad, g, b, li.lds_bytes, stream, p, a); break;
        case kWalkBvh: hipLaunchKernelGGL(records ? k_cam_bvh : k_rad_bvh, g, b, li.lds_bytes, stream, p, a); break;
        case kWalkChunk:
            if (records) hipLaunchKernelGGL(sph ? k_cam_chunk<true> : k_cam_chunk<false>, g, b, li.lds_bytes, stream, p, a);
            else hipLaunchKernelGGL(sph ? k_rad_chunk<true> : k_rad_chunk<false>, g, b, li.lds_bytes, stream, p, a);
            break;
    }
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_rad_sum, dim3((uint32_t)((blocks64 + 3u) / 4u)), dim3(256), 0, stream, a);
    if (info) *info = li;
    return (int)hipGetLastError();
}

}  // namespace rb
