// rb_runtime.cpp -- the C-ABI runtime of librenderbaby_hip.so (include/rb_abi.h): create, update, render, iterator,
// multi-device, stats and debug.  The queries and the denoiser are rb_queries.cpp's.
//
// Replaces, for the HIP backend, crates/engine-wgpu-wrapper (GpuWrapper,
// GpuBuffers, ProgressiveRenderHelper) and the host half of
// crates/engine-pathtracer/src/lib.rs: device buffers mirroring the 14 wgpu
// buffers (buffers.rs:32-61), the Change<T> state machine
// (gpu_wrapper.rs:116-300), count patch-up and uploads (:469-576), the pass loop
// (:365-426) and read-back (:432-463; the x mirror is done by the kernel's
// store).  Every entry point selects its device first (HIP's current device is
// per-thread and the reference drives the iterator from a worker thread,
// frame_buffer.rs:141-148) and reports failures as status + message instead of
// panicking.
//
// Beyond the reference (one wgpu device, one synchronous pass per frame):
//  * two frame slots (accumulation + RGBA8 each) so that the progressive iterator can run pass k+1
//    while frame k is copied to the caller;
//  * row-stripe sharding over several devices behind this same boundary -- one engine per device inside
//    one process (rb_create_multi) or one process per device (rb_comm_init_rank) -- with ONE RCCL gather
//    of the RGBA8 stripes to the root per delivered frame; rccl_gather.cpp.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "rb_engine.hpp"

static thread_local std::string g_create_error;

int rb::fail(const rb_engine* e, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (e) {
        std::lock_guard<std::mutex> g(e->err_mu);
        e->error = buf;
    } else {
        g_create_error = buf;
    }
    return code;
}

namespace {

using rb::copy_error, rb::ensure_prepared, rb::make_params, rb::require_ready;   // declared in rb_engine.hpp: rb_queries.cpp calls them too

// grow_resolution -- buffers.rs:171-180 (+ the stripe geometry of the sharded case)
int resize_frame(rb_engine* e, uint32_t w, uint32_t h, const rb::ShardLayout& rows) {
    const uint64_t px = static_cast<uint64_t>(w) * rows.padded;
    if (px >= (1ull << 31)) return rb::fail(e, RB_ERR_INVALID_UNIFORMS, "frame of %u x %u pixels is too large", w, h);
    // the frame's buffers are about to be replaced: launches queued on the engine's stream and, joined into it, on the
    // accumulate stream may still use them
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    e->spec_valid = false;
    e->cur = 0;
    e->slot[1].accum.release();   // the run-ahead slot is (re)allocated when the iterator first needs it
    e->slot[1].rgba.release();
    rb::FrameSlot& s = e->slot[0];
    HIP_TRY(e, s.accum.resize(px * 4));
    HIP_TRY(e, s.rgba.resize(px));
    if (px) {
        HIP_TRY(e, hipMemsetAsync(s.accum.ptr, 0, px * 16, e->stream));
        HIP_TRY(e, hipMemsetAsync(s.rgba.ptr, 0, px * 4, e->stream));
    }
    return RB_OK;
}

int upload_textures(rb_engine* e, const rb_texture* t, size_t count) {
    std::vector<uint32_t> data;
    std::vector<rb_texture_info> info;
    uint32_t offset = 0;
    for (size_t i = 0; i < count; ++i) {  // process_textures, buffers.rs:151-168
        const size_t n = static_cast<size_t>(t[i].width) * t[i].height;
        info.push_back(rb_texture_info{offset, t[i].width, t[i].height, 0});
        data.insert(data.end(), t[i].rgba_data, t[i].rgba_data + n);
        offset += t[i].width * t[i].height;
    }
    int rc = rb::upload(e, e->tex_data, data.data(), data.size(), true);
    if (rc) return rc;
    rc = rb::upload(e, e->tex_info, info.data(), info.size(), true);
    if (rc) return rc;
    HIP_TRY(e, hipStreamSynchronize(e->stream));  // `data`/`info` are locals
    return RB_OK;
}

// The lean scan's records of the spheres just uploaded (one per element of e->spheres, the zero-filled element of an
// empty field included, so that no count a launch may carry reads past them).
int prep_sphere_scan(rb_engine* e) {
    const size_t n = e->spheres.count;
    HIP_TRY(e, e->sph_scan.resize(n * 4));
    int rc = rb::launch_prep_sphere_scan(e->spheres.ptr, static_cast<uint32_t>(n), e->sph_scan.ptr, e->stream);
    if (rc) return rb::fail(e, RB_ERR_DEVICE, "sphere scan prep launch failed: %s", hipGetErrorString(static_cast<hipError_t>(rc)));
    return RB_OK;
}

// The sift's group table of a single-node tree, from the node and the prepared triangles as the device holds them (the f32
// edges the kernels use; at most kSiftMaxSlots records of 64 B come back).  Any other tree, or a list with nothing to reject,
// leaves the table empty.
int prep_tri_filter(rb_engine* e) {
    e->sift_table = rb::SiftTable{};
    if (!e->tri_filter || rb::kernel_of(e->opt) != RB_KERNEL_STREAM || rb::node_count(e->sc) != 1u || !e->nodes.ptr || !e->ptris.ptr) return RB_OK;
    rb_bvh_node node{};
    HIP_TRY(e, hipMemcpyAsync(&node, e->nodes.ptr, sizeof node, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    const uint32_t len = e->sc.n_indices, first = node.first_primitive, count = node.primitive_count;
    const uint32_t end = (static_cast<uint64_t>(first) + count < len) ? first + count : len;   // guard :331, as intersect_bvh has it
    if (first >= end || end - first > rb::kSiftMaxSlots) return RB_OK;
    std::vector<rb::PrepTri> list(end);   // indexed by slot; only [first, end) is read
    HIP_TRY(e, hipMemcpyAsync(list.data() + first, e->ptris.ptr + first, (end - first) * sizeof(rb::PrepTri), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    rb::SiftTable tb;
    rb::build_sift_table(list.data(), first, end, tb);
    if (!rb::sift_pays(tb)) return RB_OK;
    HIP_TRY(e, e->sift_groups.resize(tb.groups.size()));
    HIP_TRY(e, hipMemcpyAsync(e->sift_groups.ptr, tb.groups.data(), tb.groups.size() * sizeof(rb::SiftGroup), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));   // `tb.groups` is pageable host memory
    e->sift_table = std::move(tb);
    return RB_OK;
}

// the box of the spheres just uploaded (centre -+ |radius|, outward): part of the sift's origin region.  A spheres field is taken
// whole (apply_field uploads `src, n` as the new array), so these are all the spheres the device holds.
void keep_sphere_box(rb_engine* e, const rb_sphere* s, size_t n) {
    e->sph_box_any = false;
    for (size_t i = 0; s && i < n; ++i) {
        const float r = std::fabs(s[i].radius) * 1.0001f;
        for (int k = 0; k < 3; ++k) {
            const float lo = s[i].center[k] - r, hi = s[i].center[k] + r;
            e->sph_box[k] = e->sph_box_any ? std::min(e->sph_box[k], lo) : lo;
            e->sph_box[3 + k] = e->sph_box_any ? std::max(e->sph_box[3 + k], hi) : hi;
        }
        e->sph_box_any = true;
    }
}

int prep_materials(rb_engine* e, rb_material* first, size_t stride, size_t n) {
    if (!first || n == 0) return RB_OK;
    int rc = rb::launch_prep_materials(first, static_cast<uint32_t>(stride), static_cast<uint32_t>(n), e->stream);
    if (rc) return rb::fail(e, RB_ERR_DEVICE, "material prep launch failed: %s", hipGetErrorString(static_cast<hipError_t>(rc)));
    return RB_OK;
}

// the host's copy of a mesh field of n elements just uploaded, or its staleness (ensure_host_mesh fetches it if need be)
template <typename T>
void keep_host_copy(rb_engine* e, const void* src, size_t n, std::vector<T>& copy, size_t& len, bool& stale) {
    if (!rb::mesh_walks(e->opt).host_mesh) return;
    len = n;
    stale = rb::host_copy_can_wait(e, n);
    if (stale) std::vector<T>().swap(copy);
    else copy.assign(static_cast<const T*>(src), static_cast<const T*>(src) + n);
}

// One field of an update as the plan decides it (rb_update_plan.hpp): what needs the device or the engine.  The field's
// facts change when its buffer has been written.
int apply_field(rb_engine* e, rb::Field f, const rb::UpdatePlan& pl, const rb_config* cfg) {
    using namespace rb;
    if (f == kUniforms) {   // gpu_wrapper.rs:122-136 / :165-192
        if (pl.act[f] == Act::Take) {
            const rb_uniforms* u = static_cast<const rb_uniforms*>(cfg->uniforms.ptr);
            if (pl.resize || e->slot[0].accum.ptr == nullptr)
                if (const int rc = resize_frame(e, u->width, u->height, pl.frame)) return rc;
            e->prh.total_samples = u->total_samples;  // ProgressiveRenderHelper::update (:47-52)
            e->prh.total_passes = (u->total_samples + e->prh.samples_per_pass - 1) / e->prh.samples_per_pass;
        }
        commit_field(e->sc, pl, cfg, f);
        return RB_OK;
    }
    if (pl.act[f] == Act::None) return RB_OK;
    const bool del = pl.act[f] == Act::Delete;
    const void* src = del ? nullptr : field_of(cfg, f).ptr;
    const size_t n = del ? 0 : field_of(cfg, f).count;
    int rc = RB_OK;
    switch (f) {
        case kSpheres: rc = upload(e, e->spheres, src, n, true); break;
        case kUvs: rc = upload(e, e->uvs, src, n, true); break;
        case kMeshes: rc = upload(e, e->meshes, src, n, true); break;
        case kLights: rc = upload(e, e->lights, src, n, !del); break;   // delete_lights: no element at all (buffers.rs:389-391)
        case kNodes: rc = upload(e, e->nodes, src, n, true); break;
        case kIndices: rc = upload(e, e->indices, src, n, true); break;
        case kTriangles: rc = upload(e, e->tris, src, n, true); break;
        case kTextures: rc = upload_textures(e, static_cast<const rb_texture*>(src), n); break;
        default: break;
    }
    if (rc) return rc;
    commit_field(e->sc, pl, cfg, f);
    switch (f) {
        case kSpheres:
            rc = prep_materials(e, &e->spheres.ptr->material, sizeof(rb_sphere), n);
            if (!rc) rc = prep_sphere_scan(e);
            keep_sphere_box(e, static_cast<const rb_sphere*>(src), n);
            if (!rc) rc = build_sphere_bvh(e, static_cast<const rb_sphere*>(src), n);
            break;
        case kMeshes: rc = prep_materials(e, &e->meshes.ptr->material, sizeof(rb_mesh), n); break;
        case kLights: rc = prep_materials(e, e->lights.ptr ? &e->lights.ptr->material : nullptr, sizeof(rb_point_light), e->sc.n_lights); break;
        case kNodes:
            e->prep_dirty = true;
            e->tree = {n ? "caller" : "", 0.0f};
            break;
        case kIndices:
            e->prep_dirty = true;
            keep_host_copy(e, src, n, e->host_indices, e->host_index_len, e->host_indices_stale);
            break;
        case kTriangles:
            e->prep_dirty = true;
            keep_host_copy(e, src, n, e->host_tris, e->host_tri_len, e->host_tris_stale);
            break;
        default: break;
    }
    return rc;
}

}  // namespace

// ---- what rb_queries.cpp shares with this file (rb_engine.hpp)
int rb::ensure_prepared(rb_engine* e) {
    // shader.wgsl:336 skips triangle ids >= uniforms.bvh_triangle_count: the prepared triangles carry that
    // guard as their `valid` word, so they depend on the (patched) count as well as on the buffers
    const uint32_t tri_count = rb::triangle_count(e->sc);
    if (!e->prep_dirty && e->prep_tri_count == tri_count) return RB_OK;
    const uint32_t len = e->sc.n_indices;  // arrayLength(&bvh_indices) >= 1
    HIP_TRY(e, e->ptris.resize(len));
    HIP_TRY(e, e->pshade.resize(len));
    int rc = rb::launch_prep_tris(e->tris.ptr, tri_count, e->indices.ptr, len, e->ptris.ptr, e->pshade.ptr, e->stream);
    if (rc) return rb::fail(e, RB_ERR_DEVICE, "prep kernel launch failed: %s", hipGetErrorString(static_cast<hipError_t>(rc)));
    e->prep_dirty = false;
    e->prep_tri_count = tri_count;
    // ---- the mesh walk's tree (rb_accel.cpp): the chunked walk's if wanted, else the library's own if wanted
    e->chunk.rec = e->own.rec = {};
    rc = rb::build_chunk_tree(e, tri_count);
    if (!rc && !e->chunk.rec.built()) rc = rb::build_own_tree(e, tri_count);
    return rc ? rc : prep_tri_filter(e);
}

rb::KParams rb::make_params(rb_engine* e, uint32_t first_pass, uint32_t n_passes, int src, int dst) {
    rb::KParams p{};
    p.u = e->sc.uniforms;
    p.u.spheres_count = rb::spheres_count(e->sc);
    p.u.bvh_node_count = rb::node_count(e->sc);
    p.u.bvh_triangle_count = rb::triangle_count(e->sc);
    p.spheres = e->spheres.ptr;
    p.sph_scan = e->sph_scan.ptr;
    p.lights = e->lights.ptr;
    p.meshes = e->meshes.ptr;
    p.nodes = e->nodes.ptr;
    p.indices = e->indices.ptr;
    p.tris = e->tris.ptr;
    p.ptris = e->ptris.ptr;
    p.pshade = e->pshade.ptr;
    p.uvs = e->uvs.ptr;
    p.tex_data = e->tex_data.ptr;
    p.tex_info = e->tex_info.ptr;
    p.srgb_lut = e->srgb_lut.ptr;
    p.accum_in = e->slot[src].accum.ptr;
    p.accum_out = e->slot[dst].accum.ptr;
    p.out_rgba = e->slot[dst].rgba.ptr;
    p.counters = e->counters.ptr;
    p.queue = e->queue.ptr;
    p.n_lights = e->sc.n_lights;
    p.n_meshes = e->sc.n_meshes;
    p.index_len = e->sc.n_indices;
    p.n_uvs = e->sc.n_uvs;
    p.n_tex = e->sc.n_tex;
    p.first_pass = first_pass;
    p.n_passes = n_passes;
    p.samples_per_pass = e->prh.samples_per_pass;
    const rb::ShardLayout rows = e->sc.layout(e->sc.height);
    p.shard_rank = rows.rank;
    p.shard_count = rows.count;
    p.stripe_rows = rows.stripe;
    p.local_rows = e->sc.local_rows;
    p.colors = e->colors.ptr;
    // stack_depth: the largest need of the walks a launch can run, each of which must fit the column (rb_internal.hpp)
    p.stack_depth = rb::accel_params(e, p);
    e->stack_depth_covers = p.stack_depth <= rb::kStackDepth;
    p.blocks_per_cu = e->opt._reserved[0];
    // the caller's reservation size: a multiple of 64 items, at most 4096 (the launcher's own range; beyond it the
    // 32-bit queue arithmetic of the stream kernels could wrap and hand items out twice)
    p.queue_batch = e->opt._reserved[2] ? std::min<uint32_t>(((std::min<uint32_t>(e->opt._reserved[2], 4096u) + 63u) / 64u) * 64u, 4096u) : 0u;
    p.no_leaf_stepping = e->opt._reserved[3];
    p.lds_mode = e->opt._reserved[4];
    // The flat kernels' precondition ("Scenes that carry no u, v").  The lights come into it with the ground:
    // only a ground hit leaves use_texture set where no mesh or sphere material has a texture, and a light that wins after it is
    // sampled with its own index.  Trees the plain non-MULTI walk never sees establish nothing.
    const bool single = p.u.bvh_node_count <= 1u && p.sph_nodes == nullptr && !e->trace_uv;
    p.no_uv = (single && e->sc.no_uv && (e->sc.untex_lights || p.u.ground_enabled == 0u)) ? 1u : 0u;
    // The sift ("The triangle sift"): the table of this node's list, and the region of this launch's origins --
    // the table's triangles, the camera and the spheres.  Anything else a ray may start from is outside it and takes every slot.
    if (single && p.u.bvh_node_count == 1u && !e->sift_table.groups.empty() && e->sift_groups.ptr) {
        float extra[2][6];
        uint32_t n_extra = 0;
        for (int k = 0; k < 3; ++k) extra[0][k] = extra[0][3 + k] = p.u.camera.pos[k];
        n_extra++;
        if (e->sph_box_any && p.u.spheres_count > 0u) std::memcpy(extra[n_extra++], e->sph_box, sizeof e->sph_box);
        const rb::SiftRegion r = rb::sift_region(e->sift_table, extra, n_extra);
        if (r.on) {
            p.sift = 1u;
            p.sift_groups = reinterpret_cast<const float*>(e->sift_groups.ptr);
            p.sift_block_ends = e->sift_table.block_ends;
            for (int k = 0; k < 3; ++k) p.sift_lo[k] = r.lo[k], p.sift_hi[k] = r.hi[k];
            p.sift_kp = r.kp, p.sift_ks = r.ks, p.sift_kt = r.kt, p.sift_kd = r.kd;
            p.sift_rmax = r.rmax;
        }
    }
    return p;
}

int rb::require_ready(rb_engine* e) {
    if (!e->sc.initialized) return rb::fail(e, RB_ERR_NOT_INITIALIZED, "engine has not received its first update");
    if (!e->scene_valid) return rb::fail(e, RB_ERR_DEVICE, "the last update failed half-way on the device; send the scene again");
    if (!e->sc.have_uniforms) return rb::fail(e, RB_ERR_UNIFORMS_NOT_INITIALIZED, "Uniforms must be initialized");
    return RB_OK;
}

// a part's error text as its group's
void rb::copy_error(rb_engine* g, const rb_engine* part) {
    std::string msg;
    {
        std::lock_guard<std::mutex> l(part->err_mu);
        msg = part->error;
    }
    std::lock_guard<std::mutex> l(g->err_mu);
    g->error = "device " + std::to_string(part->device) + ": " + msg;
}

namespace {

int clear_accum(rb_engine* e) {
    const size_t px = static_cast<size_t>(e->sc.width) * e->sc.padded_rows;
    e->spec_valid = false;
    if (px) HIP_TRY(e, hipMemsetAsync(e->slot[e->cur].accum.ptr, 0, px * 16, e->stream));
    return RB_OK;
}

int accumulate_timing(rb_engine* e) {
    float ms = 0.0f;
    if (e->last_launches > 0) {
        HIP_TRY(e, hipEventSynchronize(e->ev_end));   // behind the join: every event of the group, on either stream, is over
        HIP_TRY(e, hipEventElapsedTime(&ms, e->ev_begin, e->ev_end));
    }
    e->last_dispatch_ms = ms;
    if (e->timing_pending) {
        e->stats.kernel_ms += ms;
        for (uint32_t i = 0; i + 4 <= e->ev_used; i += 4) {
            float t = 0.0f, a = 0.0f;
            HIP_TRY(e, hipEventElapsedTime(&t, e->ev_pool[i], e->ev_pool[i + 1]));
            HIP_TRY(e, hipEventElapsedTime(&a, e->ev_pool[i + 2], e->ev_pool[i + 3]));
            e->stats.trace_ms += t;
            e->stats.accumulate_ms += a;
        }
        e->timing_pending = false;
    }
    return RB_OK;
}

// Colour-buffer budget of the stream kernels (one float4 per (pixel, sample) of a launch chunk): the caller's
// figure, else 4 GiB but never more than half of what the device has free right now -- a library that sits behind a GUI
// should not take 34 GB for a 1080p frame.  A frame that does not fit is traced in two halves of the budget by turns
// (rb_color_plan.hpp): sixteen launches per C2 frame, each accumulated underneath the next one's trace.
uint64_t color_budget_bytes(rb_engine* e) {
    if (e->opt._reserved[1]) return static_cast<uint64_t>(e->opt._reserved[1]) << 20;
    if (e->color_budget == 0) {   // asked once per update: hipMemGetInfo is a driver round trip, and the iterator dispatches per pass
        uint64_t budget = 4ull << 30;
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget = std::min<uint64_t>(budget, (free_b + e->colors.count * sizeof(float)) / 2);
        e->color_budget = std::max<uint64_t>(budget, 1ull << 20);
    }
    return e->color_budget;
}

// The stream kernels' colour buffer for a group of n_passes passes and the plan it serves (rb_color_plan.hpp): passes per
// launch and one or two parts of one float4 per (pixel, sample) of a launch.  If the device cannot give that, halves the
// launch.  Allocates (lazily: the first dispatch, or rb_reserve).  k_queue and k_pixel have no colour buffer: their plan is
// the caller's passes per launch.
int reserve_colors(rb_engine* e, uint32_t n_passes, rb::ColorPlan* plan_out) {
    rb::ColorPlan pl;
    pl.chunk = e->opt.passes_per_launch ? e->opt.passes_per_launch : n_passes;
    if (rb::kernel_of(e->opt) == RB_KERNEL_STREAM && n_passes != 0 && e->sc.width != 0 && e->sc.local_rows != 0) {
        const uint64_t tiles = static_cast<uint64_t>((e->sc.width + 7) / 8) * ((e->sc.local_rows + 7) / 8);
        const uint64_t per_pass = tiles * 64ull * e->prh.samples_per_pass;  // items per pass
        pl = rb::plan_colors(per_pass, n_passes, e->opt.passes_per_launch, color_budget_bytes(e) / 16ull);
        if (pl.chunk == 0) return rb::fail(e, RB_ERR_INVALID_UNIFORMS, "frame too large for one launch");
        for (;;) {
            // a buffer about to be replaced may still be read by the accumulate stream: every group ends joined into the
            // engine's stream, so that one is the one to wait for
            if (e->colors.ptr && !e->colors.serves(pl.floats(per_pass))) HIP_TRY(e, hipStreamSynchronize(e->stream));
            const hipError_t st = e->colors.reserve(pl.floats(per_pass));
            if (st == hipSuccess) break;
            (void)hipGetLastError();  // clear the sticky out-of-memory status
            if (st != hipErrorOutOfMemory || !rb::halve(pl))
                return rb::fail(e, RB_ERR_DEVICE, "colour buffer of %llu bytes: %s", static_cast<unsigned long long>(pl.floats(per_pass) * 4ull),
                            hipGetErrorString(st));
        }
        e->color_part_floats = static_cast<size_t>(per_pass * pl.chunk * 4ull);
    }
    *plan_out = pl;
    return RB_OK;
}

// One launch group: passes [first_pass, first_pass + n_passes) on top of slot `src`, into slot `dst`, cut into launches by
// `pl`.  k_queue and k_pixel: one kernel per launch on the engine's stream.  The stream kernels: launch i is k_trace(i),
// which fills a colour part, and k_accumulate(i), which sums that part into the accumulation in sample order.  With one
// part both follow each other on the engine's stream.  With two parts launch i uses part i % 2, and three streams share the
// work: k_trace(i) goes to the engine's stream (even i) or to trace_stream (odd i), each with its own queue words, so that
// the persistent grid of launch i + 1 fills the wave slots the tail of launch i vacates; k_accumulate(i) goes to
// accum_stream, where it runs underneath k_trace(i + 1) in the slots that one leaves.  What must hold:
//  1. Part reuse.  k_trace(i + 2) starts after k_accumulate(i) has finished: its stream waits on ev_accumulated[i % 2]
//     before it is launched.  (It is also behind k_trace(i) on the same stream: the queue words are free.)
//  2. The accumulation chain.  k_accumulate(i) reads the accumulation k_accumulate(i - 1) wrote (`src` for the first launch,
//     `dst` after): both are on accum_stream, in order, each behind ev_traced of its own launch.  Before the first launch
//     accum_stream and trace_stream wait on ev_top, recorded on the engine's stream at the top of the group: the memset of a
//     clear, uploads, ensure_prepared's kernels, the previous group and whatever else was queued earlier come first.
//  3. The join.  After the last launch the engine's stream waits on the last accumulate's event, which is behind every
//     accumulate and hence every trace launch of the group; ev_end and the slot's `done` are recorded behind that wait.  So
//     everything that follows a dispatch on the engine's stream -- read-backs, rb_sync, the queries, the denoiser's guide
//     build, the RCCL gather, the next dispatch (also the run-ahead one into the other slot), rb_clear, rb_update -- stays
//     ordered without knowing that other streams exist.
//  4. Buffers.  No colour part, accumulation or RGBA buffer is freed or reallocated while another stream may touch it:
//     reserve_colors, resize_frame and rb_destroy wait for the engine's stream (hence, by 3, for the others) first.  A
//     launch that fails mid-group leaves all three streams idle before dispatch returns its error.
//  5. Timing keeps its meaning.  trace_ms: the sum of begin -> end of each trace launch on its stream (consecutive launches
//     overlap by their tails, so the sum can exceed the group's time); accumulate_ms: the sum of begin -> end of each
//     accumulate on its stream, the begin recorded behind the wait, so that waiting for the trace is not counted -- an
//     accumulate that shares the device with the next trace takes as long as that lets it; last_dispatch_ms: ev_begin ->
//     ev_end across the join.
//  6. RB_FLAG_STATS.  Only the trace kernels count, with atomics: concurrency changes nothing.
// Host side, k_accumulate(i) is queued before k_trace(i + 1).
int queue_group(rb_engine* e, uint32_t first_pass, uint32_t n_passes, int src, int dst, const rb::ColorPlan& pl) {
    const uint32_t kernel = rb::kernel_of(e->opt);
    const bool stats = (e->opt.flags & RB_FLAG_STATS) != 0;
    const bool two_phase = kernel == RB_KERNEL_STREAM;
    const bool overlap = two_phase && pl.parts == 2;
    hipStream_t acc = overlap ? e->accum_stream : e->stream;
    HIP_TRY(e, hipEventRecord(e->ev_begin, e->stream));
    if (overlap) {   // (2)
        HIP_TRY(e, hipEventRecord(e->ev_top, e->stream));
        HIP_TRY(e, hipStreamWaitEvent(acc, e->ev_top, 0));
        HIP_TRY(e, hipStreamWaitEvent(e->trace_stream, e->ev_top, 0));
    }
    uint32_t launches = 0;
    e->ev_used = 0;
    for (uint32_t done = 0; done < n_passes;) {
        const uint32_t n = std::min(pl.chunk, n_passes - done);
        const uint32_t part = overlap ? launches % 2u : 0u;   // the colour part, the trace stream and the queue words of this launch
        hipStream_t ts = part ? e->trace_stream : e->stream;
        // the first chunk resumes `src`; later chunks of the same group continue in `dst`
        rb::KParams p = make_params(e, first_pass + done, n, done == 0 ? src : dst, dst);
        if (!e->stack_depth_covers) return rb::fail(e, RB_ERR_DEVICE, "internal: a traversal is deeper than its LDS stack column (%u entries)", p.stack_depth);
        if (two_phase) p.colors = e->colors.ptr + part * e->color_part_floats;
        p.queue = e->queue.ptr + part * rb::kQueueWords;
        rb::LaunchInfo li{};
        // per-chunk timing events (first 256 chunks of a group; later ones only count in the total)
        hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
        if (e->ev_used + 4 <= 1024) {
            while (e->ev_pool.size() < e->ev_used + 4) {
                hipEvent_t x;
                HIP_TRY(e, hipEventCreate(&x));
                e->ev_pool.push_back(x);
            }
            for (int i = 0; i < 4; ++i) ev[i] = e->ev_pool[e->ev_used + i];
            e->ev_used += 4;
        }
        if (overlap && launches >= 2) HIP_TRY(e, hipStreamWaitEvent(ts, e->ev_accumulated[part], 0));   // (1)
        if (ev[0]) HIP_TRY(e, hipEventRecord(ev[0], ts));
        int rc = rb::launch_render(p, kernel, stats, ts, &li);
        if (rc) return rb::fail(e, RB_ERR_DEVICE, "render kernel launch failed: %s", hipGetErrorString(static_cast<hipError_t>(rc)));
        if (ev[1]) HIP_TRY(e, hipEventRecord(ev[1], ts));
        if (overlap) {
            HIP_TRY(e, hipEventRecord(e->ev_traced[part], ts));
            HIP_TRY(e, hipStreamWaitEvent(acc, e->ev_traced[part], 0));
        }
        if (ev[2]) HIP_TRY(e, hipEventRecord(ev[2], acc));
        if (two_phase) {
            rc = rb::launch_accumulate(p, acc);
            if (rc) return rb::fail(e, RB_ERR_DEVICE, "accumulate kernel launch failed: %s", hipGetErrorString(static_cast<hipError_t>(rc)));
        }
        if (ev[3]) HIP_TRY(e, hipEventRecord(ev[3], acc));
        if (overlap) HIP_TRY(e, hipEventRecord(e->ev_accumulated[part], acc));
        if (li.kernel_name) e->last_kernel_name = li.kernel_name, e->last_trace_form = li.trace_form;
        done += n;
        launches++;
    }
    if (overlap) HIP_TRY(e, hipStreamWaitEvent(e->stream, e->ev_accumulated[(launches - 1u) % 2u], 0));   // (3)
    HIP_TRY(e, hipEventRecord(e->ev_end, e->stream));
    HIP_TRY(e, hipEventRecord(e->slot[dst].done, e->stream));
    e->last_launches = launches;
    e->timing_pending = true;
    e->stats.launches += launches;
    return RB_OK;
}

// dispatch_compute_progressive without the host sync -- gpu_wrapper.rs:365-400: passes
// [first_pass, first_pass + n_passes) on top of slot `src`, into slot `dst` (the same slot, or the other one
// when the iterator runs a pass ahead).
int dispatch(rb_engine* e, uint32_t first_pass, uint32_t n_passes, int src, int dst) {
    int rc = ensure_prepared(e);
    if (rc) return rc;
    if (n_passes == 0 || e->sc.width == 0 || e->sc.local_rows == 0) {
        e->last_launches = 0;
        return RB_OK;
    }
    if (e->timing_pending) {  // fold the previous group's events before they are recorded again
        rc = accumulate_timing(e);
        if (rc) return rc;
    }
    rb::ColorPlan pl;
    rc = reserve_colors(e, n_passes, &pl);
    if (rc) return rc;
    rc = queue_group(e, first_pass, n_passes, src, dst, pl);
    if (rc) {   // (4) a group cut short: nothing of it is left running, on either stream, when the caller sees the error
        (void)hipStreamSynchronize(e->accum_stream);
        (void)hipStreamSynchronize(e->trace_stream);
        (void)hipStreamSynchronize(e->stream);
        e->last_launches = 0;
        e->timing_pending = false;
    }
    return rc;
}

// Copies the committed frame's RGBA8 rows (local stripe order when sharded) to caller memory: the host waits
// for the launches that produced the slot, then a blocking copy.  The engine's stream is non-blocking, so a
// pass the iterator has already started on the OTHER slot keeps running underneath this copy.
int read_slot_rgba(rb_engine* e, int slot, uint8_t* out) {
    if (!out) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "rgba_out is NULL");
    const uint32_t sc = e->opt.shard_count > 1 ? e->opt.shard_count : 1;
    const size_t bytes = static_cast<size_t>(e->sc.width) * 4 * (sc == 1 ? e->sc.height : e->sc.padded_rows);
    if (bytes == 0) return RB_OK;
    // Page-locked destination (rb_host_alloc, or memory the caller registered with HIP): a DMA on the copy
    // stream straight into it, behind the slot's event -- no staging, no host-side copy.
    hipPointerAttribute_t attr{};
    if (hipPointerGetAttributes(&attr, out) == hipSuccess && attr.type == hipMemoryTypeHost) {
        HIP_TRY(e, hipStreamWaitEvent(e->copy_stream, e->slot[slot].done, 0));
        HIP_TRY(e, hipMemcpyAsync(out, e->slot[slot].rgba.ptr, bytes, hipMemcpyDeviceToHost, e->copy_stream));
        HIP_TRY(e, hipStreamSynchronize(e->copy_stream));
        return RB_OK;
    }
    (void)hipGetLastError();  // an unregistered pointer makes the query fail: that is the ordinary case
    HIP_TRY(e, hipEventSynchronize(e->slot[slot].done));
    HIP_TRY(e, hipMemcpy(out, e->slot[slot].rgba.ptr, bytes, hipMemcpyDeviceToHost));
    return RB_OK;
}

int read_rgba(rb_engine* e, uint8_t* out) {
    // uploads and clears queued after the slot's last launch group must be over as well
    HIP_TRY(e, hipEventRecord(e->slot[e->cur].done, e->stream));
    return read_slot_rgba(e, e->cur, out);
}

int update_fields(rb_engine* e, const rb_config* cfg) {
    rb::UpdatePlan plan;
    std::string why;
    if (const int rc = rb::plan_update(e->sc, cfg, plan, why)) return rb::fail(e, rc, "%s", why.c_str());   // nothing has been touched: the previous scene stays live

    // ---- from here on the buffers change; a device failure half-way leaves the engine refusing to render
    e->scene_valid = false;
    e->spec_valid = false;
    e->color_budget = 0;
    e->dn_guides_valid = false;   // the denoiser's guides are this scene's and this camera's
    e->hist_base_valid = false;   // ... and so is the base the history was carried into (section 22)
    e->emit_valid = false;        // ... and the emitter table this scene's
    e->emit_cdf_valid = false;    // ... with its pick weights by power (section 23)
    for (uint32_t f = 0; f < rb::kFieldCount; ++f)
        if (const int rc = apply_field(e, static_cast<rb::Field>(f), plan, cfg)) return rc;
    if (plan.own_tree != rb::OwnTree::Keep) {   // the tree follows the triangles field (RB_FLAG_BUILD_TREE)
        const bool rebuild = plan.own_tree == rb::OwnTree::Rebuild;
        if (const int rc = rb::build_engine_tree(e, static_cast<const rb_gpu_triangle*>(rebuild ? cfg->bvh_triangles.ptr : nullptr),
                                                 rebuild ? cfg->bvh_triangles.count : 0))
            return rc;
    }
    rb::commit_end(e->sc, plan);
    e->scene_valid = true;
    return RB_OK;
}

// Inputs are borrowed only for this call: whatever update_fields has queued from the caller's
// buffers must have left them before we return -- also when it stops half-way with an error.
// (Without Create/Update uniforms the reference panics at the next use, gpu_wrapper.rs:303-329;
// here that is require_ready's error.)
int update_locked(rb_engine* e, const rb_config* cfg) {
    const int rc = update_fields(e, cfg);
    const hipError_t st = hipStreamSynchronize(e->stream);
    if (rc) return rc;
    if (st != hipSuccess) return rb::fail(e, RB_ERR_DEVICE, "hipStreamSynchronize: %s", hipGetErrorString(st));
    return RB_OK;
}

// zero the accumulation, run every pass (dispatch_compute, gpu_wrapper.rs:406-426) -- no read-back
int render_async(rb_engine* e) {
    int rc = require_ready(e);
    if (rc) return rc;
    rc = clear_accum(e);  // :407-411
    if (rc) return rc;
    e->prh.current_pass = 0;
    rc = dispatch(e, 0, e->prh.total_passes, e->cur, e->cur);
    if (rc) return rc;
    e->prh.current_pass = e->prh.total_passes ? e->prh.total_passes - 1 : 0;  // loop variable's last value (:415)
    return RB_OK;
}

int render_locked(rb_engine* e, uint8_t* rgba_out) {
    if (!rgba_out && !(e->net.nranks > 1 && e->net.rank != 0)) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "rgba_out is NULL");
    int rc = render_async(e);
    if (rc) return rc;
    if (e->net.nranks > 1) {  // one process per device: the frame is assembled on rank 0
        std::string why;
        if (rb::gather_process(e->net, e->slot[e->cur].rgba.ptr, e->sc.width, e->sc.height, e->sc.padded_rows,
                               e->sc.layout(e->sc.height).stripe, e->copy_stream, e->slot[e->cur].done,
                               rgba_out, why))
            return rb::fail(e, RB_ERR_DEVICE, "%s", why.c_str());
    } else {
        rc = read_rgba(e, rgba_out);
        if (rc) return rc;
    }
    return accumulate_timing(e);
}

// One step of the progressive iterator on one engine, without the delivery: passes [current_pass, +n) end up in
// slot[cur].  They are taken from the run-ahead slot when the previous call started exactly these passes there (and
// nothing has touched the scene or the accumulation since); then the next group is started on the other slot, so that
// it computes while the caller's frame is exchanged and copied out (frame_buffer.rs:164-221 pumps frames from a worker
// thread; lib.rs:200-205 syncs, maps and mirrors per pass).  The exchange and the read-back run on the engine's second
// stream behind the slot's event, so a sharded engine -- one process per device, or a part of a multi-device handle --
// runs ahead like a whole-frame one.
int iter_advance(rb_engine* e, uint32_t per_frame) {
    int rc = require_ready(e);
    if (rc) return rc;
    if (!e->iter_initialized) {  // lib.rs:181-192
        rc = clear_accum(e);
        if (rc) return rc;
        e->iter_initialized = true;
    }
    const uint32_t per = std::max(per_frame, 1u);
    const uint32_t n = std::min(per, e->prh.total_passes - e->prh.current_pass);
    if (e->spec_valid && e->spec_first == e->prh.current_pass && e->spec_n == n) {
        e->cur = 1 - e->cur;   // commit the pass group that has been running since the previous call
        e->spec_valid = false;
    } else {
        e->spec_valid = false;
        rc = dispatch(e, e->prh.current_pass, n, e->cur, e->cur);  // lib.rs:200-203 (n = 1 there)
        if (rc) return rc;
    }
    e->prh.current_pass += n;  // lib.rs:213
    rc = accumulate_timing(e);
    if (rc) return rc;
    // ---- run ahead: the next group on the other slot
    if (!(e->opt.flags & RB_FLAG_NO_RUN_AHEAD) && e->prh.current_pass < e->prh.total_passes) {
        rb::FrameSlot& o = e->slot[1 - e->cur];
        const size_t px = static_cast<size_t>(e->sc.width) * e->sc.padded_rows;
        if (o.accum.count != px * 4 || o.rgba.count != px) {
            HIP_TRY(e, o.accum.resize(px * 4));
            HIP_TRY(e, o.rgba.resize(px));
            // rows a sharded engine pads its stripes with are never written by a kernel: callers that read the
            // slot must not see what the allocator left there
            if (px) HIP_TRY(e, hipMemsetAsync(o.accum.ptr, 0, px * 16, e->stream));
            if (px) HIP_TRY(e, hipMemsetAsync(o.rgba.ptr, 0, px * 4, e->stream));
        }
        const uint32_t n2 = std::min(per, e->prh.total_passes - e->prh.current_pass);
        rc = dispatch(e, e->prh.current_pass, n2, e->cur, 1 - e->cur);
        if (rc) return rc;
        e->spec_valid = true;
        e->spec_first = e->prh.current_pass;
        e->spec_n = n2;
    }
    return RB_OK;
}

int iter_next_locked(rb_engine* e, uint8_t* rgba_out) {
    if (!(e->prh.current_pass < e->prh.total_passes))
        return rb::fail(e, RB_ERR_NO_MORE_FRAMES, "No more frames available");  // lib.rs:170-177
    const bool multiproc = e->net.nranks > 1;
    if (!rgba_out && !(multiproc && e->net.rank != 0)) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "rgba_out is NULL");
    int rc = iter_advance(e, e->iter_passes_per_frame);
    if (rc) return rc;
    if (multiproc) {
        std::string why;
        if (rb::gather_process(e->net, e->slot[e->cur].rgba.ptr, e->sc.width, e->sc.height, e->sc.padded_rows,
                               e->sc.layout(e->sc.height).stripe, e->copy_stream, e->slot[e->cur].done,
                               rgba_out, why))
            return rb::fail(e, RB_ERR_DEVICE, "%s", why.c_str());
        return RB_OK;
    }
    return read_slot_rgba(e, e->cur, rgba_out);  // lib.rs:205
}

rb_engine* create_single(const rb_config* cfg, const rb_options& opt) {
    if (opt.shard_count > 1 && opt.shard_rank >= opt.shard_count) {
        rb::fail(nullptr, RB_ERR_INVALID_OPTIONS, "shard_rank %u >= shard_count %u", opt.shard_rank, opt.shard_count);
        return nullptr;
    }
    if (opt.kernel > RB_KERNEL_STREAM) { rb::fail(nullptr, RB_ERR_INVALID_OPTIONS, "unknown kernel %u", opt.kernel); return nullptr; }
    if ((opt.flags & rb::kBuildTreeFlags) == rb::kBuildTreeFlags) {
        rb::fail(nullptr, RB_ERR_INVALID_OPTIONS, "RB_FLAG_BUILD_TREE and RB_FLAG_BUILD_TREE_HOST exclude each other");
        return nullptr;
    }
    int dev = opt.device;
    if (dev < 0) {
        if (hipGetDevice(&dev) != hipSuccess) { rb::fail(nullptr, RB_ERR_DEVICE, "no HIP device available"); return nullptr; }
    }
    if (hipSetDevice(dev) != hipSuccess) { rb::fail(nullptr, RB_ERR_DEVICE, "hipSetDevice(%d) failed", dev); return nullptr; }
    rb_engine* e = new rb_engine();
    e->device = dev;
    e->opt = opt;
    e->sc.own_tree = rb::builds_tree(opt);
    e->sc.shard_rank = opt.shard_rank, e->sc.shard_count = opt.shard_count, e->sc.stripe_rows = opt.stripe_rows;
    // RB_REFERENCE_WALK=1 in the environment: every engine of this process walks meshes exactly as shader.wgsl:282-392 does,
    // whatever the host program's flags say -- the escape hatch from the culled walks (whose exactness is derived and fuzzed,
    // DESIGN.md section 4.2) that needs no rebuild of the host
    if (const char* rw = std::getenv("RB_REFERENCE_WALK"); rw && rw[0] == '1')
        e->opt.flags = (e->opt.flags & ~(rb::kOwnTreeFlags | RB_FLAG_DEVICE_LBVH | RB_FLAG_CHUNK_WALK | RB_FLAG_SKIP_NEAR_DEGENERATE)) |
                       RB_FLAG_REFERENCE_WALK;
    // RB_TRACE_UV=1: this engine's plain walk keeps the kernels that carry u, v, whatever the scene (A/B runs, tests)
    if (const char* uv = std::getenv("RB_TRACE_UV"); uv && uv[0] == '1') e->trace_uv = true;
    // RB_TRI_FILTER=0: this engine's plain walk keeps the kernels whose triangle loop runs every trip (A/B runs, tests)
    if (const char* tf = std::getenv("RB_TRI_FILTER"); tf && tf[0] == '0') e->tri_filter = false;
    auto bail = [&](const char* what, hipError_t st) -> rb_engine* {
        rb::fail(nullptr, RB_ERR_DEVICE, "%s failed: %s", what, hipGetErrorString(st));
        rb_destroy(e);
        return nullptr;
    };
    hipError_t st;
    if ((st = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking)) != hipSuccess) return bail("hipStreamCreate", st);
    if ((st = hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking)) != hipSuccess) return bail("hipStreamCreate", st);
    if ((st = hipStreamCreateWithFlags(&e->accum_stream, hipStreamNonBlocking)) != hipSuccess) return bail("hipStreamCreate", st);
    if ((st = hipStreamCreateWithFlags(&e->trace_stream, hipStreamNonBlocking)) != hipSuccess) return bail("hipStreamCreate", st);
    for (hipEvent_t* x : {&e->ev_top, &e->ev_traced[0], &e->ev_traced[1], &e->ev_accumulated[0], &e->ev_accumulated[1]})
        if ((st = hipEventCreateWithFlags(x, hipEventDisableTiming)) != hipSuccess) return bail("hipEventCreate", st);
    if ((st = hipEventCreate(&e->ev_begin)) != hipSuccess) return bail("hipEventCreate", st);
    if ((st = hipEventCreate(&e->ev_end)) != hipSuccess) return bail("hipEventCreate", st);
    for (rb::FrameSlot& s : e->slot)
        if ((st = hipEventCreateWithFlags(&s.done, hipEventDisableTiming)) != hipSuccess) return bail("hipEventCreate", st);
    if ((st = e->counters.resize(rb::C_COUNT)) != hipSuccess) return bail("hipMalloc(counters)", st);
    if ((st = e->queue.resize(2 * rb::kQueueWords)) != hipSuccess) return bail("hipMalloc(queue)", st);
    if ((st = hipMemsetAsync(e->counters.ptr, 0, sizeof(unsigned long long) * rb::C_COUNT, e->stream)) != hipSuccess)
        return bail("hipMemset(counters)", st);
    // sRGB -> linear table for sample_texture's pow(c, 2.2) (shader.wgsl:185-190)
    float lut[256];
    for (int i = 0; i < 256; ++i) lut[i] = powf(static_cast<float>(i) / 255.0f, 2.2f);
    if ((st = e->srgb_lut.resize(256)) != hipSuccess) return bail("hipMalloc(lut)", st);
    if ((st = hipMemcpy(e->srgb_lut.ptr, lut, sizeof lut, hipMemcpyHostToDevice)) != hipSuccess) return bail("hipMemcpy(lut)", st);
    // ProgressiveRenderHelper::new (gpu_wrapper.rs:38-45); SAMPLES_PER_PASS = 1 (:12)
    const rb_uniforms* u = static_cast<const rb_uniforms*>(cfg->uniforms.ptr);
    e->prh.samples_per_pass = 1;
    e->prh.total_samples = u->total_samples;
    e->prh.total_passes = u->total_samples;
    e->prh.current_pass = 0;
    return e;
}

bool check_create(const rb_config* cfg) {
    g_create_error.clear();
    // GpuBuffers::new panics unless these are Create (buffers.rs:74-97)
    int rc = rb::check_tags(cfg, g_create_error);
    if (!rc) rc = rb::check_first_config(cfg, g_create_error);
    return rc == RB_OK;
}

rb_engine* create_impl(const rb_config* cfg, const rb_options* opt_in) {
    if (!check_create(cfg)) return nullptr;
    rb_options opt{};
    opt.device = -1;
    if (opt_in) opt = *opt_in;
    return create_single(cfg, opt);
}

// ------------------------------------------------------------------ several devices, one handle ----
#define PART_TRY(g, part, call)            \
    do {                                   \
        rb::set_device(part);              \
        const int _rc = (call);            \
        if (_rc) {                         \
            copy_error((g), (part));       \
            return _rc;                    \
        }                                  \
    } while (0)

int group_update(rb_engine* g, const rb_config* cfg) {
    for (auto& p : g->parts) PART_TRY(g, p.get(), update_locked(p.get(), cfg));
    rb_engine* p0 = g->parts[0].get();
    g->sc.width = p0->sc.width;
    g->sc.height = p0->sc.height;
    g->sc.have_uniforms = p0->sc.have_uniforms;
    g->sc.initialized = p0->sc.initialized;
    g->prh = p0->prh;
    return RB_OK;
}

// the one exchange step: every part's RGBA8 stripes to the root device, de-interleaved there, then read back
int group_deliver(rb_engine* g, uint8_t* rgba_out, bool fold_timing) {
    std::vector<rb::GatherSource> src;
    for (auto& p : g->parts) src.push_back(rb::GatherSource{p->device, p->copy_stream, p->slot[p->cur].done, p->slot[p->cur].rgba.ptr});
    rb_engine* p0 = g->parts[0].get();
    std::string why;
    if (rb::gather_group(g->net, src, p0->sc.width, p0->sc.height, p0->sc.padded_rows, p0->sc.layout(p0->sc.height).stripe, rgba_out, why))
        return rb::fail(g, RB_ERR_DEVICE, "%s", why.c_str());
    // (the iterator folds a group's timing when it commits it: waiting for the events here would wait for the pass
    // that has just been started ahead)
    if (fold_timing)
        for (auto& p : g->parts) PART_TRY(g, p.get(), accumulate_timing(p.get()));
    return RB_OK;
}

int group_render(rb_engine* g, uint8_t* rgba_out) {
    if (!rgba_out) return rb::fail(g, RB_ERR_NULL_ARGUMENT, "rgba_out is NULL");
    for (auto& p : g->parts) PART_TRY(g, p.get(), render_async(p.get()));  // all devices render concurrently
    g->prh = g->parts[0]->prh;
    return group_deliver(g, rgba_out, true);
}

int group_iter_next(rb_engine* g, uint8_t* rgba_out) {
    rb_engine* p0 = g->parts[0].get();
    if (!(p0->prh.current_pass < p0->prh.total_passes)) return rb::fail(g, RB_ERR_NO_MORE_FRAMES, "No more frames available");
    if (!rgba_out) return rb::fail(g, RB_ERR_NULL_ARGUMENT, "rgba_out is NULL");
    for (auto& pp : g->parts) PART_TRY(g, pp.get(), iter_advance(pp.get(), g->iter_passes_per_frame));   // every part runs ahead
    g->prh = p0->prh;
    return group_deliver(g, rgba_out, false);
}

}  // namespace

// ============================================================== C ABI ======
extern "C" {

rb_engine* rb_create(const rb_config* cfg) { return create_impl(cfg, nullptr); }
rb_engine* rb_create_ex(const rb_config* cfg, const rb_options* opt) { return create_impl(cfg, opt); }

rb_engine* rb_create_multi(const rb_config* cfg, const rb_options* opt_in, const int32_t* devices, uint32_t n_devices) {
    if (!check_create(cfg)) return nullptr;
    if (!devices || n_devices == 0 || n_devices > 64) {
        rb::fail(nullptr, RB_ERR_INVALID_OPTIONS, "rb_create_multi needs 1..64 devices");
        return nullptr;
    }
    rb_options opt{};
    if (opt_in) opt = *opt_in;
    if (opt.shard_count > 1) {
        rb::fail(nullptr, RB_ERR_INVALID_OPTIONS, "rb_create_multi shards by itself: leave shard_rank / shard_count zero");
        return nullptr;
    }
    std::unique_ptr<rb_engine> g(new rb_engine());
    g->opt = opt;
    g->device = devices[0];
    for (uint32_t r = 0; r < n_devices; ++r) {
        rb_options po = opt;
        po.device = devices[r];
        po.shard_rank = r;
        po.shard_count = n_devices;
        rb_engine* p = create_single(cfg, po);
        if (!p) {   // g_create_error is set
            rb_destroy(g.release());
            return nullptr;
        }
        g->parts.emplace_back(p);
    }
    std::vector<int> devs(devices, devices + n_devices);
    std::string why;
    if (rb::gather_init_group(g->net, devs, (opt.flags & RB_FLAG_GATHER_PEER_COPY) != 0u, why)) {
        rb_destroy(g.release());
        rb::fail(nullptr, RB_ERR_DEVICE, "%s", why.c_str());
        return nullptr;
    }
    rb_engine* out = g.release();
    return out;
}

int rb_comm_available(void) {
    std::string why;
    if (rb::gather_available(why)) {
        g_create_error = why;
        return RB_ERR_DEVICE;
    }
    return RB_OK;
}

int rb_comm_unique_id(uint8_t id_out[RB_COMM_ID_BYTES]) {
    if (!id_out) return RB_ERR_NULL_ARGUMENT;
    std::string why;
    if (rb::gather_unique_id(id_out, why)) {
        g_create_error = why;
        return RB_ERR_DEVICE;
    }
    return RB_OK;
}

int rb_comm_init_rank(rb_engine* e, const uint8_t id[RB_COMM_ID_BYTES], uint32_t rank, uint32_t nranks) {
    if (!e || !id) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    if (rb::is_group(e)) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "rb_comm_init_rank is for single-device engines");
    const uint32_t sc = e->opt.shard_count > 1 ? e->opt.shard_count : 1;
    if (nranks != sc || rank != (sc > 1 ? e->opt.shard_rank : 0u))
        return rb::fail(e, RB_ERR_INVALID_OPTIONS, "communicator rank %u of %u does not match shard %u of %u", rank, nranks,
                    e->opt.shard_rank, sc);
    rb::set_device(e);
    std::string why;
    if (rb::gather_init_rank(e->net, e->device, id, rank, nranks, why)) return rb::fail(e, RB_ERR_DEVICE, "%s", why.c_str());
    return RB_OK;
}

int rb_comm_info(rb_engine* e, uint32_t* rccl_ranks, uint32_t* rccl_rank, float* last_gather_ms) {
    if (!e) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    std::string why;
    if (rb::gather_comm_info(e->net, rccl_ranks, rccl_rank, why)) return rb::fail(e, RB_ERR_DEVICE, "%s", why.c_str());
    if (last_gather_ms) *last_gather_ms = e->net.last_ms;
    return RB_OK;
}

void rb_destroy(rb_engine* e) {
    if (!e) return;
    if (rb::is_group(e)) {
        for (auto& p : e->parts) {
            rb::set_device(p.get());
            if (p->stream) (void)hipStreamSynchronize(p->stream);
        }
        rb::gather_destroy(e->net);
        for (auto& p : e->parts) rb_destroy(p.release());
        delete e;
        return;
    }
    rb::set_device(e);
    // every launch, copy and event record of this engine was queued on its stream or, joined into it before the
    // dispatch returned, on the accumulate stream: when they have drained nothing on the device refers to the buffers,
    // events or communicator any more
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    if (e->accum_stream) {
        (void)hipStreamSynchronize(e->accum_stream);
        (void)hipStreamDestroy(e->accum_stream);
    }
    if (e->trace_stream) {
        (void)hipStreamSynchronize(e->trace_stream);
        (void)hipStreamDestroy(e->trace_stream);
    }
    if (e->copy_stream) {
        (void)hipStreamSynchronize(e->copy_stream);
        (void)hipStreamDestroy(e->copy_stream);
    }
    rb::gather_destroy(e->net);
    if (e->ev_begin) (void)hipEventDestroy(e->ev_begin);
    if (e->ev_end) (void)hipEventDestroy(e->ev_end);
    for (hipEvent_t x : {e->ev_top, e->ev_traced[0], e->ev_traced[1], e->ev_accumulated[0], e->ev_accumulated[1]})
        if (x) (void)hipEventDestroy(x);
    for (rb::FrameSlot& s : e->slot)
        if (s.done) (void)hipEventDestroy(s.done);
    for (hipEvent_t x : e->ev_pool) (void)hipEventDestroy(x);
    for (rb::StageTimer* t : {&e->t_query, &e->t_generator, &e->t_sh, &e->t_depth, &e->t_lm_surfels, &e->t_lm_resolve, &e->t_guides,
                              &e->t_filter, &e->t_history})
        t->destroy();
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
}

const char* rb_last_error(const rb_engine* e) {
    if (!e) return g_create_error.c_str();
    // a copy per calling thread: another thread's failing call may replace the engine's text at any moment
    // (the reference's GUI polls from its own thread), and a pointer into that string would dangle
    thread_local std::string mine;
    {
        std::lock_guard<std::mutex> g(e->err_mu);
        mine = e->error;
    }
    return mine.c_str();
}

int rb_update(rb_engine* e, const rb_config* cfg) {
    if (!e) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    if (rb::is_group(e)) return group_update(e, cfg);
    rb::set_device(e);
    return update_locked(e, cfg);
}

int rb_render(rb_engine* e, uint8_t* rgba_out) {
    if (!e) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    if (rb::is_group(e)) return group_render(e, rgba_out);
    rb::set_device(e);
    return render_locked(e, rgba_out);
}

int rb_render_config(rb_engine* e, const rb_config* cfg, uint8_t* rgba_out) {
    if (!e) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    if (rb::is_group(e)) {
        const int rc = group_update(e, cfg);
        return rc ? rc : group_render(e, rgba_out);
    }
    rb::set_device(e);
    int rc = update_locked(e, cfg);
    if (rc) return rc;
    return render_locked(e, rgba_out);
}

int rb_iter_begin(rb_engine* e, const rb_config* cfg) {
    if (!e) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    if (rb::is_group(e)) {
        int rc = group_update(e, cfg);
        if (rc) return rc;
        for (auto& p : e->parts) {
            PART_TRY(e, p.get(), require_ready(p.get()));
            p->prh.current_pass = 0;
            p->iter_initialized = false;
        }
        e->prh = e->parts[0]->prh;
        return RB_OK;
    }
    rb::set_device(e);
    int rc = update_locked(e, cfg);
    if (rc) return rc;
    rc = require_ready(e);
    if (rc) return rc;
    e->prh.current_pass = 0;       // lib.rs:91
    e->iter_initialized = false;   // RaytracerFrameIterator::new (lib.rs:144-150)
    e->spec_valid = false;
    return RB_OK;
}

int rb_iter_has_next(rb_engine* e) {
    if (!e) return 0;
    std::lock_guard<std::mutex> lock(e->mu);
    const rb_engine* s = rb::is_group(e) ? e->parts[0].get() : e;
    return s->prh.current_pass < s->prh.total_passes ? 1 : 0;  // lib.rs:153-156
}

int rb_iter_next(rb_engine* e, uint8_t* rgba_out) {
    if (!e) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    if (rb::is_group(e)) return group_iter_next(e, rgba_out);
    rb::set_device(e);
    return iter_next_locked(e, rgba_out);
}

void rb_iter_destroy(rb_engine* e) { (void)e; }  // lib.rs:231-233: logs only

int rb_iter_set_passes_per_frame(rb_engine* e, uint32_t n) {
    if (!e) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    e->iter_passes_per_frame = n;
    return RB_OK;
}

int rb_get_size(const rb_engine* e, uint32_t* width, uint32_t* height) {
    if (!e) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(const_cast<rb_engine*>(e)->mu);
    if (!e->sc.have_uniforms) return rb::fail(e, RB_ERR_UNIFORMS_NOT_INITIALIZED, "Uniforms must be initialized");  // gpu_wrapper.rs:313,321
    if (width) *width = e->sc.width;
    if (height) *height = e->sc.height;
    return RB_OK;
}

int rb_clear(rb_engine* e) {
    if (!e) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    if (rb::is_group(e)) {
        for (auto& p : e->parts) {
            PART_TRY(e, p.get(), require_ready(p.get()));
            PART_TRY(e, p.get(), clear_accum(p.get()));
        }
        return RB_OK;
    }
    rb::set_device(e);
    int rc = require_ready(e);
    if (rc) return rc;
    return clear_accum(e);
}

int rb_dispatch(rb_engine* e, uint32_t first_pass, uint32_t n_passes) {
    if (!e) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    if (rb::is_group(e)) {
        for (auto& p : e->parts) {
            PART_TRY(e, p.get(), require_ready(p.get()));
            p->spec_valid = false;
            PART_TRY(e, p.get(), dispatch(p.get(), first_pass, n_passes, p->cur, p->cur));
        }
        return RB_OK;
    }
    rb::set_device(e);
    int rc = require_ready(e);
    if (rc) return rc;
    e->spec_valid = false;
    return dispatch(e, first_pass, n_passes, e->cur, e->cur);
}

int rb_reserve(rb_engine* e, uint32_t n_passes) {
    if (!e) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    auto one = [&](rb_engine* p) {
        rb::set_device(p);
        int rc = require_ready(p);
        if (!rc) rc = ensure_prepared(p);
        rb::ColorPlan pl;
        if (!rc) rc = reserve_colors(p, n_passes, &pl);
        if (!rc && hipStreamSynchronize(p->stream) != hipSuccess) rc = rb::fail(p, RB_ERR_DEVICE, "synchronise failed");
        return rc;
    };
    if (rb::is_group(e)) {
        for (auto& p : e->parts) PART_TRY(e, p.get(), one(p.get()));
        return RB_OK;
    }
    return one(e);
}

int rb_sync(rb_engine* e) {
    if (!e) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    if (rb::is_group(e)) {
        for (auto& p : e->parts) {
            rb::set_device(p.get());
            HIP_TRY(e, hipStreamSynchronize(p->stream));
        }
        return RB_OK;
    }
    rb::set_device(e);
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return RB_OK;
}

int rb_read_rgba(rb_engine* e, uint8_t* rgba_out) {
    if (!e) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    if (rb::is_group(e)) {
        if (!rgba_out) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "rgba_out is NULL");
        return group_deliver(e, rgba_out, false);
    }
    rb::set_device(e);
    int rc = require_ready(e);
    if (rc) return rc;
    return read_rgba(e, rgba_out);
}

int rb_read_accumulation(rb_engine* e, float* accum_out) {
    if (!e) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    if (!accum_out) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "accum_out is NULL");
    if (rb::is_group(e)) {
        // debugging / checkpoint path: every part's rows through the host, in image order
        rb_engine* p0 = e->parts[0].get();
        const uint32_t w = p0->sc.width, h = p0->sc.height;
        std::vector<float> tmp(static_cast<size_t>(w) * p0->sc.padded_rows * 4);
        for (auto& part : e->parts) {
            rb_engine* p = part.get();
            const rb::ShardLayout rows = p->sc.layout(h);
            PART_TRY(e, p, require_ready(p));
            HIP_TRY(e, hipStreamSynchronize(p->stream));
            HIP_TRY(e, hipMemcpy(tmp.data(), p->slot[p->cur].accum.ptr, tmp.size() * sizeof(float), hipMemcpyDeviceToHost));
            for (uint32_t lr = 0; lr < p->sc.padded_rows; ++lr) {
                const uint32_t y = rows.global_row(lr);
                if (y < h) std::memcpy(accum_out + static_cast<size_t>(y) * w * 4, tmp.data() + static_cast<size_t>(lr) * w * 4, static_cast<size_t>(w) * 16);
            }
        }
        return RB_OK;
    }
    rb::set_device(e);
    int rc = require_ready(e);
    if (rc) return rc;
    const uint32_t rows = (e->opt.shard_count > 1) ? e->sc.padded_rows : e->sc.height;
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    HIP_TRY(e, hipMemcpy(accum_out, e->slot[e->cur].accum.ptr, static_cast<size_t>(e->sc.width) * rows * 16, hipMemcpyDeviceToHost));
    return RB_OK;
}

void* rb_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return p;
}

void rb_host_free(void* p) {
    if (p) (void)hipHostFree(p);
}

int rb_device_rgba(rb_engine* e, void** d_ptr, size_t* bytes) {
    if (!e) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    if (rb::is_group(e)) {  // the assembled frame on the root device (valid after a render / iterator step)
        if (d_ptr) *d_ptr = rb::gather_frame_ptr(e->net);
        if (bytes) *bytes = static_cast<size_t>(e->sc.width) * e->sc.height * 4;
        return RB_OK;
    }
    if (d_ptr) *d_ptr = e->slot[e->cur].rgba.ptr;
    if (bytes) *bytes = static_cast<size_t>(e->sc.width) * e->sc.padded_rows * 4;
    return RB_OK;
}

int rb_local_rows(const rb_engine* e, uint32_t* rows, uint32_t* padded_rows) {
    if (!e) return RB_ERR_NULL_ARGUMENT;
    const rb::ShardLayout l = e->sc.layout(e->sc.height);   // a group handle delivers whole frames: its facts name no shard
    if (rows) *rows = l.owned;
    if (padded_rows) *padded_rows = l.padded;
    return RB_OK;
}

int rb_global_row(const rb_engine* e, uint32_t local_row, uint32_t* global_row) {
    if (!e || !global_row) return RB_ERR_NULL_ARGUMENT;
    *global_row = e->sc.layout(e->sc.height).global_row(local_row);
    return RB_OK;
}

int rb_shard_layout(uint32_t height, uint32_t shard_rank, uint32_t shard_count, uint32_t stripe_rows,
                    uint32_t* owned_rows, uint32_t* padded_rows) {
    const rb::ShardLayout l = rb::shard_layout(height, shard_rank, shard_count, stripe_rows);
    if (shard_rank >= l.count) return RB_ERR_INVALID_OPTIONS;
    if (owned_rows) *owned_rows = l.owned;
    if (padded_rows) *padded_rows = l.padded;
    return RB_OK;
}

uint32_t rb_shard_global_row(uint32_t shard_rank, uint32_t shard_count, uint32_t stripe_rows, uint32_t local_row) {
    return rb::shard_layout(0, shard_rank, shard_count, stripe_rows).global_row(local_row);
}

static int part_stats(rb_engine* e, rb_stats* out);

int rb_get_stats(rb_engine* e, rb_stats* out) {
    if (!e || !out) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    if (rb::is_group(e)) {  // work counters add up; the devices run side by side, so times are the slowest part's
        rb_stats sum{};
        for (auto& p : e->parts) {
            rb_stats s{};
            PART_TRY(e, p.get(), part_stats(p.get(), &s));
            sum.segments += s.segments; sum.paths += s.paths; sum.nodes_popped += s.nodes_popped;
            sum.tris_tested += s.tris_tested; sum.spheres_tested += s.spheres_tested;
            sum.lights_tested += s.lights_tested; sum.mesh_hits += s.mesh_hits;
            sum.launches = std::max(sum.launches, s.launches);
            sum.kernel_ms = std::max(sum.kernel_ms, s.kernel_ms);
            sum.trace_ms = std::max(sum.trace_ms, s.trace_ms);
            sum.accumulate_ms = std::max(sum.accumulate_ms, s.accumulate_ms);
        }
        *out = sum;
        return RB_OK;
    }
    rb::set_device(e);
    return part_stats(e, out);
}

static int part_stats(rb_engine* e, rb_stats* out) {
    unsigned long long c[rb::C_COUNT];
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    {
        const int rc = accumulate_timing(e);
        if (rc) return rc;
    }
    HIP_TRY(e, hipMemcpy(c, e->counters.ptr, sizeof c, hipMemcpyDeviceToHost));
    e->stats.segments = c[rb::C_SEGMENTS];
    e->stats.paths = c[rb::C_PATHS];
    e->stats.nodes_popped = c[rb::C_NODES];
    e->stats.tris_tested = c[rb::C_TRIS];
    e->stats.spheres_tested = c[rb::C_SPHERES];
    e->stats.lights_tested = c[rb::C_LIGHTS];
    e->stats.mesh_hits = c[rb::C_MESH_HITS];
    *out = e->stats;
    return RB_OK;
}

static int part_reset_stats(rb_engine* e);

int rb_reset_stats(rb_engine* e) {
    if (!e) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    if (rb::is_group(e)) {
        for (auto& p : e->parts) PART_TRY(e, p.get(), part_reset_stats(p.get()));
        return RB_OK;
    }
    rb::set_device(e);
    return part_reset_stats(e);
}

static int part_reset_stats(rb_engine* e) {
    {   // a launch group whose events have not been read yet belongs to the period that ends here
        const int rc = accumulate_timing(e);
        if (rc) return rc;
    }
    HIP_TRY(e, hipMemsetAsync(e->counters.ptr, 0, sizeof(unsigned long long) * rb::C_COUNT, e->stream));
    e->stats = rb_stats{};
    return RB_OK;
}

int rb_last_dispatch_ms(rb_engine* e, float* ms) {
    if (!e || !ms) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    if (rb::is_group(e)) {
        *ms = 0.0f;
        for (auto& p : e->parts) {
            PART_TRY(e, p.get(), accumulate_timing(p.get()));
            *ms = std::max(*ms, p->last_dispatch_ms);
        }
        return RB_OK;
    }
    rb::set_device(e);
    int rc = accumulate_timing(e);
    if (rc) return rc;
    *ms = e->last_dispatch_ms;
    return RB_OK;
}

const char* rb_version(void) { return "renderbaby-hip 0.3 (gfx950)"; }

const char* rb_last_kernel_name(const rb_engine* e) {
    if (!e) return "";
    return rb::is_group(e) ? e->parts[0]->last_kernel_name : e->last_kernel_name;
}

uint32_t rb_debug_trace_form(const rb_engine* e) {
    if (!e) return 0u;
    return rb::is_group(e) ? e->parts[0]->last_trace_form : e->last_trace_form;
}

int rb_device_name(int device, char* buf, size_t buf_len) {
    if (!buf || buf_len == 0) return RB_ERR_NULL_ARGUMENT;
    hipDeviceProp_t prop;
    if (device < 0 && hipGetDevice(&device) != hipSuccess) return RB_ERR_DEVICE;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return RB_ERR_DEVICE;
    snprintf(buf, buf_len, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    return RB_OK;
}

int rb_debug_walk_profile(uint64_t out64[64], int reset) {
    if (!out64) return RB_ERR_NULL_ARGUMENT;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "counter width");
    if (hipDeviceSynchronize() != hipSuccess) return RB_ERR_DEVICE;
    return rb::debug_walk_profile(reinterpret_cast<unsigned long long*>(out64), reset) == 0 ? RB_OK : RB_ERR_DEVICE;
}

int rb_debug_tri_filter(rb_engine* e, const float* rays, uint32_t n, uint32_t* out, uint32_t* list2) {
    if (!e || !rays || !out || !list2) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> g(e->mu);
    rb::set_device(e);
    if (int rc = require_ready(e)) return rc;
    if (int rc = ensure_prepared(e)) return rc;
    const rb::KParams p = make_params(e, 0, 0, e->cur, e->cur);
    // (a table may stand while the scene carries u, v: only the flat kernels sift, plan_launch)
    if (p.sift == 0u || p.no_uv == 0u) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "this engine's scene does not sift its triangle list");
    if (n == 0u) return RB_OK;
    if (n > (1u << 22)) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "at most 2^22 rays");
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    list2[0] = e->sift_table.first, list2[1] = e->sift_table.end;
    return rb::debug_tri_filter(p, rays, n, list2[0], list2[1], out);
}

}  // extern "C"
