"""The launch plan of the stream kernels' trace launch (renderbaby_amd/csrc/rb_launch_plan.hpp): which walk runs, grid, LDS,
reservation size, division reciprocals and where the work queue starts.  Plain integer arithmetic, so it is compiled into a
stand-alone program under AddressSanitizer and UBSan and run on the host; no GPU, and nothing is loaded into Python.

The properties are the ones the kernels rely on (ItemQueue, ColorRing, udiv_magic), checked over a sweep of frames, sample
counts, walks, grid densities, forced batches and CU counts; the worked cases are launch_render's arithmetic at 256 CUs."""
import os
import subprocess
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = textwrap.dedent(r'''
    #include <cstdio>
    #include <cstring>
    #include <vector>
    #include "rb_launch_plan.hpp"
    using namespace rb;
    static int failures = 0;
    // what a failing check was looking at: a label, or the sweep's tuple
    static const char* g_what = "";
    static const KParams* g_p = nullptr;
    static uint32_t g_cus = 0, g_stats = 0;
    static void fail(int line, const char* text) {
        if (failures++ >= 20) return;
        std::printf("line %d: %s   [%s", line, text, g_what);
        if (g_p) std::printf(" %u x %u, passes %u x %u, nodes %u, chunk %d fast %d sph %d, no_leaf_stepping %u, lds_mode %u, blocks_per_cu %u, queue_batch %u, %u CUs, stats %u",
                             g_p->u.width, g_p->local_rows, g_p->n_passes, g_p->samples_per_pass, g_p->u.bvh_node_count, g_p->chunk_nodes != nullptr, g_p->fast_nodes != nullptr,
                             g_p->sph_nodes != nullptr, g_p->no_leaf_stepping, g_p->lds_mode, g_p->blocks_per_cu, g_p->queue_batch, g_cus, g_stats);
        std::puts("]");
    }
    #define CHECK(c) do { if (!(c)) fail(__LINE__, #c); } while (0)

    // the product's constants (rb_kernels.hip, rb_device_chunk.hpp)
    static const LaunchConsts K = {256u, 4u, 3ull << 23, 64u * 32u + 64u * 8u + 128u * 4u, 64u * 32u + 64u * 8u + 64u * 4u + 128u * 4u + 128u * 4u, 4u, 5u, true};
    static const size_t kMaxLds = 160u * 1024u;   // gfx950
    static int dummy;

    // the scenes the runtime can hand over
    enum Kind { SINGLE, SINGLE_SPH, CHUNK, CHUNK_SPH, FAST, REF_SMALL, REF_LARGE, CHUNK_NO_STEP, SPH_NO_STEP, REF_NO_LDS, KINDS };
    static KParams params(uint32_t w, uint32_t rows, uint32_t S, int kind, uint32_t bpc, uint32_t qb) {
        KParams p{};
        p.u.width = w, p.local_rows = rows, p.stack_depth = 32, p.blocks_per_cu = bpc, p.queue_batch = qb;
        p.n_passes = S == 1024u ? 16u : 1u, p.samples_per_pass = S == 1024u ? 64u : S;
        const bool mesh = kind >= CHUNK && kind != SPH_NO_STEP;
        p.u.bvh_node_count = !mesh ? 1u : kind == REF_LARGE ? 100000u : 31u;
        p.index_len = kind == REF_LARGE ? 200000u : 64u;
        if (kind == CHUNK || kind == CHUNK_SPH || kind == CHUNK_NO_STEP) p.chunk_nodes = reinterpret_cast<const ChunkNode*>(&dummy);
        if (kind == FAST) p.fast_nodes = reinterpret_cast<const SphereNode*>(&dummy);
        if (kind == SINGLE_SPH || kind == CHUNK_SPH || kind == SPH_NO_STEP) p.sph_nodes = reinterpret_cast<const SphereNode4*>(&dummy);
        if (kind == CHUNK_NO_STEP || kind == SPH_NO_STEP) p.no_leaf_stepping = 1u;
        if (kind == REF_NO_LDS) p.lds_mode = 1u;
        return p;
    }
    static uint64_t items_of(const KParams& p) {
        return (uint64_t)((p.u.width + 7u) / 8u) * ((p.local_rows + 7u) / 8u) * 64u * p.n_passes * p.samples_per_pass;
    }

    // udiv_magic as the kernels read it (rb_device_shade.hpp): q = the high word of n * magic is exact or one low
    static uint32_t udiv_magic(uint32_t n, uint32_t d, uint32_t magic, uint32_t& rem) {
        uint32_t q = (uint32_t)(((uint64_t)n * magic) >> 32);
        uint32_t r = n - q * d;
        if (r >= d) q++, r -= d;
        rem = r;
        return q;
    }

    // ItemQueue::band_item
    static bool band_item(const LaunchPlan& pl, uint32_t g, uint32_t local, uint32_t total, uint32_t& item) {
        const uint32_t stripe = pl.queue_region, k = local / stripe;
        const uint64_t it = ((uint64_t)k * pl.queue_groups + g) * stripe + (local - k * stripe);
        if (it >= total) return false;
        item = (uint32_t)it;
        return true;
    }
    // every item of the launch handed out exactly once: the waves' own first reservations, then the queue word(s) to the end
    static void walk_items(const KParams& p, const LaunchPlan& pl) {
        const uint32_t total = (uint32_t)items_of(p), batch = pl.queue_batch, wpb = pl.li.block / 64u;
        std::vector<unsigned char> seen(total, 0);
        auto take = [&](uint32_t first) {
            const uint32_t end = (total - first < batch) ? total : first + batch;
            for (uint32_t it = first; it < end; it++) seen[it]++;
        };
        uint32_t word[kQueueGroups];
        for (uint32_t g = 0; g < kQueueGroups; g++) word[g] = pl.queue_start[g];
        for (uint32_t blk = 0; blk < pl.li.grid; blk++)
            for (uint32_t wv = 0; wv < wpb; wv++) {
                if (pl.queue_groups <= 1u) {
                    const uint64_t first = (uint64_t)(blk * wpb + wv) * batch;
                    if (first < total) take((uint32_t)first);
                } else {
                    const uint64_t first = (uint64_t)((blk / pl.queue_groups) * wpb + wv) * batch;
                    uint32_t it = 0;
                    if (first < 0xFFFFFFFFull && band_item(pl, blk % pl.queue_groups, (uint32_t)first, total, it)) take(it);
                }
            }
        if (pl.queue_groups <= 1u) {
            for (uint32_t b = word[0]; b < total; b += batch) take(b);
        } else {
            for (uint32_t g = 0; g < pl.queue_groups; g++)
                for (uint32_t it = 0; band_item(pl, g, word[g], total, it); word[g] += batch) take(it);
        }
        uint32_t wrong = 0;
        for (uint32_t it = 0; it < total; it++) wrong += seen[it] != 1;
        CHECK(wrong == 0);
        // the item decode: it / 64 -> (tile, sample) -> (tx, ty)
        const uint32_t S = p.n_passes * p.samples_per_pass, tiles_x = (p.u.width + 7u) / 8u;
        uint32_t bad = 0;
        for (uint32_t it = 0; it < total; it += 64u) {
            uint32_t smp, tx;
            const uint32_t tile = udiv_magic(it >> 6, S, pl.magic_S, smp);
            const uint32_t ty = udiv_magic(tile, tiles_x, pl.magic_tiles_x, tx);
            bad += tile != (it >> 6) / S || smp != (it >> 6) % S || ty != tile / tiles_x || tx != tile % tiles_x;
        }
        CHECK(bad == 0);
    }

    static void check_plan(const KParams& p, bool stats, uint32_t cus, const LaunchPlan& pl) {
        const uint64_t items = items_of(p), S = (uint64_t)p.n_passes * p.samples_per_pass;
        const bool plain = pl.variant == kTracePlain;
        CHECK(items > 0 && pl.li.grid > 0);
        CHECK(pl.li.block == (pl.variant == kTraceBvhLds ? 1024u : K.trace_block));
        // grid: never beyond the device's residency, never beyond the work
        const uint32_t residency = pl.variant == kTraceBvhLds ? 1u : p.blocks_per_cu ? p.blocks_per_cu : pl.variant == kTraceFast ? 4u
                                   : pl.variant == kTraceSph ? K.sph_waves : pl.variant == kTraceChunk ? K.chunk_waves : 8u;
        CHECK((uint64_t)pl.li.grid * pl.li.block <= (uint64_t)cus * residency * pl.li.block);
        CHECK(pl.li.grid <= (items + pl.li.block - 1u) / pl.li.block);
        CHECK(pl.li.lds_bytes <= kMaxLds);
        // batch: whole 64-item rows, inside the clamps unless the caller fixed it
        const uint64_t batch = pl.queue_batch;
        CHECK(batch % 64u == 0u && batch >= 64u);
        if (p.queue_batch) CHECK(batch == p.queue_batch);
        else CHECK(batch <= (plain ? 512u : 4096u));
        // the colour ring needs reservations of whole multiples of kRingRows rows: staged exactly then
        if (plain && pl.plain != kPlainMulti) CHECK((pl.plain == kPlainStaged) == (batch % (K.ring_rows * 64u) == 0u));
        if (plain) CHECK((pl.plain == kPlainMulti) == (p.u.bvh_node_count > 1u || p.sph_nodes != nullptr));
        CHECK(pl.big == (plain && pl.plain != kPlainMulti && !stats && items >= K.many_items));
        // the queue starts behind the waves' own first reservations; nothing is truncated on the way to 32 bits
        const uint64_t wpb = pl.li.block / 64u, waves = pl.li.grid * wpb;
        if (pl.queue_groups == 1u) {
            CHECK(pl.queue_region == 0u);
            CHECK((uint64_t)pl.queue_start[0] == waves * batch);
        } else {
            CHECK(!plain && pl.queue_groups == kQueueGroups && pl.li.grid >= kQueueGroups);
            const uint64_t region = pl.queue_region, row_items = (uint64_t)((p.u.width + 7u) / 8u) * 64u * S;
            CHECK(region % batch == 0u && region >= 8u * batch && region >= 4u * row_items && region < (1ull << 30));
            CHECK(region - batch < std::max<uint64_t>(4u * row_items, 8u * batch));   // the smallest such stripe: no bits lost
            CHECK(items >= 4u * kQueueGroups * region);                              // at least four stripes per band
            uint64_t blocks = 0;
            for (uint32_t g = 0; g < kQueueGroups; g++) {
                uint64_t blocks_g = 0;
                for (uint32_t blk = g; blk < pl.li.grid; blk += kQueueGroups) blocks_g++;
                CHECK((uint64_t)pl.queue_start[g] == blocks_g * wpb * batch && pl.queue_start[g] <= 0x7FFFFFFFu);
                blocks += blocks_g;
            }
            CHECK(blocks == pl.li.grid);
        }
        CHECK((uint64_t)pl.magic_S == (S > 1u ? (1ull << 32) / S : 0xFFFFFFFFull));
        const uint64_t tiles_x = (p.u.width + 7u) / 8u;
        CHECK((uint64_t)pl.magic_tiles_x == (tiles_x > 1u ? (1ull << 32) / tiles_x : 0xFFFFFFFFull));
    }

    struct Want { uint32_t w, rows, S; int kind; uint32_t qb; const char* name; uint32_t grid, batch, groups, region, start; PlainKind plain; bool big; };

    int main() {
        // ---- the sweep
        std::vector<uint32_t> ws, hs;
        for (uint32_t w = 1; w <= 2000; w += 211) ws.push_back(w);
        for (uint32_t w : {2u, 7u, 8u, 9u, 24u, 63u, 64u, 65u, 1280u, 1283u, 1920u, 2000u}) ws.push_back(w);
        for (uint32_t h = 1; h <= 1100; h += 157) hs.push_back(h);
        for (uint32_t h : {7u, 8u, 9u, 40u, 720u, 1024u, 1080u, 1100u}) hs.push_back(h);
        unsigned long long plans = 0, walked = 0, banded = 0;
        for (uint32_t w : ws) for (uint32_t h : hs) for (uint32_t S : {1u, 2u, 3u, 15u, 16u, 64u, 1024u}) {
            if ((uint64_t)((w + 7u) / 8u) * ((h + 7u) / 8u) * 64u * S >= (1ull << 31)) continue;   // a launch stays below 2^31 items (rb_color_plan.hpp)
            for (int kind = 0; kind < KINDS; kind++) for (uint32_t bpc : {0u, 1u, 8u}) for (uint32_t qb : {0u, 64u, 192u, 256u, 4096u})
            for (uint32_t cus : {1u, 8u, 256u}) for (int stats = 0; stats < 2; stats++) {
                const KParams p = params(w, h, S, kind, bpc, qb);
                const LaunchPlan pl = plan_launch(p, stats != 0, cus, kMaxLds, K);
                g_what = "sweep", g_p = &p, g_cus = cus, g_stats = (uint32_t)stats;
                check_plan(p, stats != 0, cus, pl);
                plans++, banded += pl.queue_groups > 1u;
                if (stats == 0 && (items_of(p) <= (1u << 13) || (pl.queue_groups > 1u && items_of(p) <= (1u << 16)))) walk_items(p, pl), walked++;
            }
        }
        // small banded plans walked to the end, whatever the sweep met: 8 x 1024 is 128 tile rows of one tile
        for (int kind : {(int)CHUNK, (int)CHUNK_SPH, (int)SINGLE_SPH, (int)FAST, (int)REF_NO_LDS}) for (uint32_t S : {2u, 3u, 16u}) for (uint32_t cus : {8u, 256u})
        for (uint32_t w : {8u, 24u}) {
            const KParams p = params(w, 1024, S, kind, 0, 0);
            const LaunchPlan pl = plan_launch(p, false, cus, kMaxLds, K);
            g_what = "small banded plans", g_p = &p, g_cus = cus, g_stats = 0;
            CHECK(pl.queue_groups == kQueueGroups);
            check_plan(p, false, cus, pl);
            walk_items(p, pl), walked++;
        }
        g_what = "the sweep itself", g_p = nullptr;
        CHECK(plans > 300000 && walked > 1000 && banded > 10000);
        // nothing to launch
        { const LaunchPlan pl = plan_launch(params(0, 40, 1, SINGLE, 0, 0), false, 256, kMaxLds, K); CHECK(pl.li.grid == 0u); }

        // ---- worked cases: 256 CUs, stack_depth 32, blocks_per_cu 0
        const Want want[] = {
            {1920, 1080, 64, SINGLE, 0, "k_trace", 2048, 512, 1, 0, 4194304, kPlainStaged, true},
            {1920, 1080, 64, SINGLE, 192, "k_trace", 2048, 192, 1, 0, 1572864, kPlainDirect, true},
            {1920, 1080, 2, SINGLE, 0, "k_trace", 1024, 64, 1, 0, 262144, kPlainDirect, false},       // sparse: half the grid
            {64, 40, 1, SINGLE, 0, "k_trace", 10, 64, 1, 0, 2560, kPlainDirect, false},
            {8, 8, 1, SINGLE, 0, "k_trace", 1, 64, 1, 0, 256, kPlainDirect, false},
            {1920, 1080, 16, CHUNK, 0, "k_trace_chunk", 1280, 64, 8, 983040, 40960, kPlainDirect, false},
            {1280, 720, 1, CHUNK, 0, "k_trace_chunk", 1280, 64, 1, 0, 327680, kPlainDirect, false},   // too few stripes to band
            {1283, 720, 3, SINGLE_SPH, 0, "k_trace_sph", 1024, 64, 1, 0, 262144, kPlainDirect, false},
        };
        const uint64_t want_items[] = {132710400, 132710400, 4147200, 2560, 64, 33177600, 921600, 2782080};
        int i = 0;
        for (const Want& c : want) {
            const KParams p = params(c.w, c.rows, c.S, c.kind, 0, c.qb);
            const LaunchPlan pl = plan_launch(p, false, 256, kMaxLds, K);
            g_what = "worked case", g_p = &p, g_cus = 256, g_stats = 0;
            CHECK(items_of(p) == want_items[i++]);
            CHECK(!std::strcmp(pl.li.kernel_name, c.name) && pl.li.grid == c.grid && pl.li.block == 256u);
            CHECK(pl.queue_batch == c.batch && pl.queue_groups == c.groups && pl.queue_region == c.region);
            for (uint32_t g = 0; g < c.groups; g++) CHECK(pl.queue_start[g] == c.start);
            if (pl.variant == kTracePlain) CHECK(pl.plain == c.plain && pl.big == c.big);
        }
        g_what = "worked cases", g_p = nullptr;
        {
            LaunchPlan pl = plan_launch(params(1920, 1080, 64, SINGLE, 0, 0), false, 256, kMaxLds, K);
            CHECK(pl.magic_S == 67108864u && pl.magic_tiles_x == 17895697u && pl.li.lds_bytes == 4u * 32u * 256u);
            CHECK(!plan_launch(params(1920, 1080, 64, SINGLE, 0, 0), true, 256, kMaxLds, K).big);   // the stats build has no 8-wave k_trace
            pl = plan_launch(params(8, 8, 1, SINGLE, 0, 0), false, 256, kMaxLds, K);
            CHECK(pl.magic_S == 0xFFFFFFFFu && pl.magic_tiles_x == 0xFFFFFFFFu);
            pl = plan_launch(params(1920, 1080, 16, CHUNK, 0, 0), false, 256, kMaxLds, K);
            CHECK(pl.li.lds_bytes == 4u * 32u * 256u + 4u * K.chunk_wave_lds && !pl.sph_tree);
            CHECK(plan_launch(params(1920, 1080, 16, CHUNK_SPH, 0, 0), false, 256, kMaxLds, K).sph_tree);
            pl = plan_launch(params(1283, 720, 3, SINGLE_SPH, 0, 0), false, 256, kMaxLds, K);
            CHECK(pl.magic_S == 1431655765u && pl.magic_tiles_x == 26676815u && pl.li.lds_bytes == 4u * 32u * 256u + 4u * K.sph_wave_lds);
        }
        // ---- the walk: chunk over fast over reference walk over sphere tree over plain
        {
            KParams p = params(64, 40, 4, CHUNK_SPH, 0, 0);
            p.fast_nodes = reinterpret_cast<const SphereNode*>(&dummy);
            auto variant = [&]() { return plan_launch(p, false, 256, kMaxLds, K).variant; };
            CHECK(variant() == kTraceChunk);
            p.chunk_nodes = nullptr;  CHECK(variant() == kTraceFast);
            p.fast_nodes = nullptr;   CHECK(variant() == kTraceBvhLds);   // a multi-node tree is walked, the sphere tree inside its kernel
            p.u.bvh_node_count = 1;   CHECK(variant() == kTraceSph);
            p.sph_nodes = nullptr;    CHECK(variant() == kTracePlain);
            // no_leaf_stepping: a multi-node tree, or the sphere tree, goes to k_trace<.., MULTI = true>, whatever trees exist
            p = params(64, 40, 4, CHUNK_NO_STEP, 0, 0);
            LaunchPlan pl = plan_launch(p, false, 256, kMaxLds, K);
            CHECK(pl.variant == kTracePlain && pl.plain == kPlainMulti && !pl.big && !std::strcmp(pl.li.kernel_name, "k_trace"));
            pl = plan_launch(params(64, 40, 4, SPH_NO_STEP, 0, 0), false, 256, kMaxLds, K);
            CHECK(pl.variant == kTracePlain && pl.plain == kPlainMulti);
            pl = plan_launch(params(1920, 1080, 64, CHUNK_NO_STEP, 0, 0), false, 256, kMaxLds, K);
            CHECK(pl.plain == kPlainMulti && !pl.big && pl.queue_batch == 512u);   // MULTI keeps one instantiation whatever the batch
            // the LDS walk exactly when lds_mode != 1 and 4 x stack bytes + 48 x (nodes + indices) fits the device's maximum
            p = params(64, 40, 4, REF_SMALL, 0, 0);
            const size_t stacks = 4u * (4u * 32u * 256u);
            p.u.bvh_node_count = 100, p.index_len = (uint32_t)((kMaxLds - stacks) / 48u) - 100u;
            pl = plan_launch(p, false, 256, kMaxLds, K);
            CHECK(pl.variant == kTraceBvhLds && pl.li.block == 1024u && pl.li.grid == 10u && pl.li.lds_bytes == stacks + 48u * (p.u.bvh_node_count + p.index_len));
            CHECK(!std::strcmp(pl.li.kernel_name, "k_trace_bvh_lds") && pl.li.lds_bytes <= kMaxLds && pl.li.lds_bytes + 48u > kMaxLds);
            p.index_len++;
            pl = plan_launch(p, false, 256, kMaxLds, K);
            CHECK(pl.variant == kTraceBvh && pl.li.block == 256u && pl.li.lds_bytes == 4u * 32u * 256u && !std::strcmp(pl.li.kernel_name, "k_trace_bvh"));
            p.index_len--, p.lds_mode = 1;
            CHECK(plan_launch(p, false, 256, kMaxLds, K).variant == kTraceBvh);
            p.lds_mode = 0;
            const size_t need = stacks + 48u * (p.u.bvh_node_count + p.index_len);
            CHECK(plan_launch(p, false, 256, need, K).variant == kTraceBvhLds && plan_launch(p, false, 256, need - 1u, K).variant == kTraceBvh);   // a device with less
            CHECK(plan_launch(p, false, 1, kMaxLds, K).li.grid == 1u);                 // one 1024-thread block per CU
        }
        if (failures) return 1;
        std::puts("ok");
        return 0;
    }
''')


def test_launch_plan_under_sanitizers(tmp_path):
    src = tmp_path / "launch_plan.cpp"
    src.write_text(SRC)
    exe = tmp_path / "launch_plan"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "renderbaby_amd", "csrc"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "ok"
