// rb_launch_plan.hpp -- every number of a stream-kernel launch: which trace walk runs, its grid, LDS and reservation size, the
// division reciprocals, and where the work queue starts (launch_render in rb_kernels.hip and launch_radiance in rb_radiance.hip
// act on it; DESIGN.md section 4, "The launch plan").  Plain arithmetic on integers: host code only, no HIP -- what the device and
// the kernel files know comes in as arguments -- so that a stand-alone program can exercise it (tests/test_launch_plan.py).
#pragma once
#include <algorithm>
#include <cstdint>

#include "rb_internal.hpp"

namespace rb {

// the constants that live in the kernel files (compile-time knobs of tools/build_variant.sh among them)
struct LaunchConsts {
    uint32_t trace_block, ring_rows;     // kTraceBlock, kRingRows
    uint64_t many_items;                 // kTraceManyItems
    uint32_t chunk_wave_lds, sph_wave_lds;   // kChunkWaveLds, kSphWaveLds
    uint32_t sph_waves, chunk_waves;     // RB_SPH_WAVES, RB_CHUNK_WAVES
    bool xcd_bands;                      // RB_XCD_BANDS
    bool flat = false;                   // the build has the flat kernels (the hand-laid trip they are written around is on)
};

// the trace walks, in the order of their names; of the plain walk the instantiation too
enum TraceVariant : uint32_t { kTracePlain, kTraceBvh, kTraceBvhLds, kTraceFast, kTraceSph, kTraceChunk };
enum PlainKind : uint32_t { kPlainMulti, kPlainStaged, kPlainDirect };   // k_trace<.., MULTI = true>, k_trace, k_trace_direct

struct LaunchPlan {
    TraceVariant variant = kTracePlain;
    LaunchInfo li{};               // block, grid (0: nothing to launch), LDS bytes, and the name rb_last_kernel_name reports
    PlainKind plain = kPlainDirect;
    bool big = false;              // the plain walk's 8-wave instantiation (never MULTI's, never a stats build's)
    bool flat = false;             // the plain walk's kernels without u, v and the texel way (k_trace_flat, k_trace_flat_direct; never MULTI's, never a stats build's)
    bool sift = false;             // the staged flat kernel with the triangle list sifted (k_trace_sift; only with flat and kPlainStaged)
    bool sph_tree = false;         // the chunked walk's SPHTREE instantiation
    uint32_t queue_batch = 0, queue_groups = 1, queue_region = 0, magic_S = 0, magic_tiles_x = 0;   // KParams' fields of these names
    uint32_t queue_start[kQueueGroups] = {};   // the queue's initial value: [0] alone, or one band-local start per group
};

// ---- the part launch_radiance shares: grid and reservation
// residency (registers): k_trace 6 waves/SIMD, the stepped walks 4
// (a launch of one or two samples per pixel -- the progressive iterator's -- leaves a wavefront of the full grid a
// few hundred items: with half the grid each regenerates paths for longer and the tail is shorter: 1080p, 1 spp,
// 0.72 instead of 0.80 ms per frame)
inline uint32_t dense_blocks_per_cu(uint64_t items, uint32_t cus) { return (items >= (uint64_t)cus * 8u * 4u * 1024u) ? 8u : 4u; }

inline uint32_t persistent_blocks(uint64_t items, uint32_t block, uint32_t cus, uint32_t blocks_per_cu) {
    uint32_t blocks = cus * blocks_per_cu;
    const uint64_t needed = (items + block - 1) / block;
    if (needed < blocks) blocks = (uint32_t)needed;
    return blocks;
}

// batch: the queue word sustains about 90 M atomics/s chip-wide, which 64-item reservations reach at 5-6 G
// items/s (C1 and C2 run there): about 8 reservations per wave, 64..512 items, a multiple of 64
// (profiles/r02_queue_batch.txt: C1 at 64 spp 17.1 -> 21.8 G segments/s)
// (the walks of trees and sphere sets hand out far fewer items per second: 64 reservations per wave, for balance)
inline uint64_t reservation(uint64_t items, uint64_t waves, bool plain) {
    uint64_t batch = items / (waves * (plain ? 8u : 64u));
    batch = (batch / 64u) * 64u;
    if (batch < 64u) batch = 64u;
    if (batch > (plain ? 512u : 4096u)) batch = (plain ? 512u : 4096u);
    return batch;
}

// reciprocal for the item decode of the stream kernels (udiv_magic): floor(2^32 / d)
inline uint32_t magic_of(uint64_t d) { return d > 1u ? (uint32_t)((1ull << 32) / d) : 0xFFFFFFFFu; }

// ---- the trace launch of RB_KERNEL_STREAM.  p: KParams as the runtime made them (of its pointers only whether chunk_nodes,
// fast_nodes and sph_nodes are present); cus, max_lds: the device's CU count and maximum dynamic LDS.
inline LaunchPlan plan_launch(const KParams& p, bool stats, uint32_t cus, size_t max_lds, const LaunchConsts& k) {
    LaunchPlan pl;
    const size_t lds = (size_t)kStackEntryBytes * p.stack_depth * 256u;
    const uint64_t tiles = (uint64_t)((p.u.width + 7u) / 8u) * ((p.local_rows + 7u) / 8u);
    const uint64_t items = tiles * 64u * p.n_passes * p.samples_per_pass;
    // which trace kernel, by what the runtime has prepared: the chunked walk (multi-node trees, the default), the
    // library's own tree (RB_FLAG_FAST_BVH), the reference-order walk (RB_FLAG_REFERENCE_WALK; from LDS when the
    // mesh fits next to the stacks: one 1024-thread block per CU, measured faster than three 256-thread blocks
    // with a copy each), the sphere tree, or the plain kernel (single-node tree, <= 64 spheres)
    const bool multi = p.u.bvh_node_count > 1u && !p.no_leaf_stepping;
    const size_t scene_lds = (size_t)p.u.bvh_node_count * 48u + (size_t)p.index_len * 48u;
    TraceVariant v = kTracePlain;
    if (multi && p.chunk_nodes != nullptr) v = kTraceChunk;
    else if (multi && p.fast_nodes != nullptr) v = kTraceFast;
    else if (multi) v = (p.lds_mode != 1u && lds * 4u + scene_lds <= max_lds) ? kTraceBvhLds : kTraceBvh;
    else if (p.sph_nodes != nullptr && !p.no_leaf_stepping) v = kTraceSph;
    static const char* const names[] = {"k_trace", "k_trace_bvh", "k_trace_bvh_lds", "k_trace_fast", "k_trace_sph", "k_trace_chunk"};
    pl.variant = v;
    pl.sph_tree = p.sph_nodes != nullptr;
    pl.li.kernel_name = names[v];
    pl.li.block = v == kTraceBvhLds ? 1024u : k.trace_block;
    pl.li.lds_bytes = v == kTraceBvhLds ? lds * 4u + scene_lds : v == kTraceChunk ? lds + (k.trace_block / 64u) * k.chunk_wave_lds
                                        : v == kTraceSph ? lds + (k.trace_block / 64u) * k.sph_wave_lds : lds;
    const uint32_t blocks_per_cu = v == kTraceBvhLds ? 1u : p.blocks_per_cu ? p.blocks_per_cu : v == kTraceFast ? 4u : v == kTraceSph ? k.sph_waves
                                                                                                   : v == kTraceChunk ? k.chunk_waves : dense_blocks_per_cu(items, cus);
    pl.li.grid = persistent_blocks(items, pl.li.block, cus, blocks_per_cu);
    if (pl.li.grid == 0) return pl;
    const uint64_t waves = (uint64_t)pl.li.grid * (pl.li.block / 64u);
    uint64_t batch = reservation(items, waves, v == kTracePlain);
    // k_trace combines its colour stores per 64-item row through a ring of kRingRows rows (ColorRing), which needs
    // reservations of whole multiples of kRingRows rows; smaller launches keep their finer reservations and store directly
    if (v == kTracePlain && batch >= 256u) batch = (batch / 256u) * 256u;
    if (p.queue_batch) batch = p.queue_batch;
    pl.queue_batch = (uint32_t)batch;
    // reciprocals for the item -> (tile, sample) -> (tx, ty) divisions (udiv_magic)
    pl.magic_S = magic_of((uint64_t)p.n_passes * p.samples_per_pass);
    pl.magic_tiles_x = magic_of((p.u.width + 7u) / 8u);
    // the queue starts behind the waves' own first reservations (ItemQueue); the walks of trees and sphere sets get one band of
    // items and one queue word per group of blocks that share an XCD
    // (stripes of about four tile rows, whole multiples of the batch; at least four stripes per band, or one word as before)
    const uint64_t row_items = (uint64_t)((p.u.width + 7u) / 8u) * 64u * p.n_passes * p.samples_per_pass;
    const uint64_t stripe = std::max<uint64_t>(((4u * row_items + batch - 1u) / batch) * batch, 8u * batch);
    const bool banded = v != kTracePlain && k.xcd_bands && pl.li.grid >= kQueueGroups && items >= 4u * kQueueGroups * stripe && stripe < (1ull << 30);
    if (banded) {
        pl.queue_groups = kQueueGroups;
        pl.queue_region = (uint32_t)stripe;
        for (uint32_t g = 0; g < kQueueGroups; g++) {
            const uint64_t blocks_g = (pl.li.grid + kQueueGroups - 1u - g) / kQueueGroups;
            pl.queue_start[g] = (uint32_t)std::min<uint64_t>(blocks_g * (pl.li.block / 64u) * batch, 0x7FFFFFFFull);   // band-local
        }
    } else {
        pl.queue_start[0] = (uint32_t)(waves * batch);   // <= 8192 waves * 4096 items
    }
    if (v == kTracePlain) {
        // MULTI: the per-segment ablation of a multi-node tree or of the sphere tree.  Else reservations of whole multiples of
        // kRingRows rows: the rows' paths are started a row at a time (ColorRing); the stats build has no 8-wave instantiation
        pl.plain = (p.u.bvh_node_count > 1u || p.sph_nodes != nullptr) ? kPlainMulti
                   : pl.queue_batch % (k.ring_rows * 64u) == 0u        ? kPlainStaged : kPlainDirect;
        pl.big = pl.plain != kPlainMulti && !stats && items >= k.many_items;
        // what the runtime has established of the scene (KParams::no_uv) picks the flat kernels
        pl.flat = k.flat && pl.plain != kPlainMulti && !stats && p.no_uv != 0u;
        // ... and what it has established of the node's list (KParams::sift, rb_tri_filter.hpp) the sifted form of the staged one
        pl.sift = pl.flat && pl.plain == kPlainStaged && p.sift != 0u && p.u.bvh_node_count == 1u;
    }
    return pl;
}

}  // namespace rb
