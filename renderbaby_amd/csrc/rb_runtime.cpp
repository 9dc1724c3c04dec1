// rb_runtime.cpp -- the C-ABI runtime of librenderbaby_hip.so (include/rb_abi.h).
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

const char* kFieldNames[9] = {"uniforms", "spheres", "uvs", "meshes", "lights",
                              "bvh_nodes", "bvh_indices", "bvh_triangles", "textures"};

const rb_field* field_at(const rb_config* c, int i) {
    const rb_field* f[9] = {&c->uniforms, &c->spheres, &c->uvs, &c->meshes, &c->lights,
                            &c->bvh_nodes, &c->bvh_indices, &c->bvh_triangles, &c->textures};
    return f[i];
}

int check_fields(rb_engine* e, const rb_config* cfg) {
    if (!cfg) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "config is NULL");
    for (int i = 0; i < 9; ++i) {
        const rb_field* f = field_at(cfg, i);
        if (f->change > RB_DELETE) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "%s: bad change tag %u", kFieldNames[i], f->change);
        if ((f->change == RB_CREATE || f->change == RB_UPDATE) && f->count > 0 && !f->ptr)
            return rb::fail(e, RB_ERR_NULL_ARGUMENT, "%s: count %zu with NULL pointer", kFieldNames[i], f->count);
    }
    if ((cfg->uniforms.change == RB_CREATE || cfg->uniforms.change == RB_UPDATE) && cfg->uniforms.count != 1)
        return rb::fail(e, RB_ERR_INVALID_UNIFORMS, "uniforms: expected exactly one rb_uniforms, got %zu", cfg->uniforms.count);
    return RB_OK;
}

// RenderConfig::validate_init -- render_config.rs:163-185
int validate_init(rb_engine* e, const rb_config* c) {
    if (c->uniforms.change != RB_CREATE) return rb::fail(e, RB_ERR_INVALID_UNIFORMS, "Invalid Uniforms");
    if (c->spheres.change != RB_CREATE) return rb::fail(e, RB_ERR_INVALID_SPHERES, "Invalid Spheres");
    if (c->uvs.change != RB_CREATE) return rb::fail(e, RB_ERR_INVALID_UVS, "Invalid UVs");
    if (c->meshes.change != RB_CREATE) return rb::fail(e, RB_ERR_INVALID_MESHES, "Invalid Meshes");
    if (c->lights.change != RB_CREATE) return rb::fail(e, RB_ERR_INVALID_LIGHTS, "Invalid Lights");
    if (c->textures.change != RB_CREATE) return rb::fail(e, RB_ERR_INVALID_TEXTURES, "Invalid Textures");
    return RB_OK;
}

bool has_data(const rb_field& f) { return f.change == RB_CREATE || f.change == RB_UPDATE; }

// RenderConfig::validate -- render_config.rs:187-268
int validate(rb_engine* e, const rb_config* c) {
    if (has_data(c->uniforms)) {
        const rb_uniforms* u = static_cast<const rb_uniforms*>(c->uniforms.ptr);
        if (!(u->camera.pane_distance >= 0.0f && u->camera.pane_distance <= 100.0f))
            return rb::fail(e, RB_ERR_PANE_DISTANCE_OUT_OF_BOUNDS, "Pane-Distance is out of bounds");
        if (!(u->camera.pane_width >= 0.0f && u->camera.pane_width <= 1000.0f))
            return rb::fail(e, RB_ERR_PANE_WIDTH_OUT_OF_BOUNDS, "Pane-Distance is out of bounds");  // sic, :631-633
        const float* d = u->camera.dir;
        const float len_sq = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        if (len_sq < 1.1920929e-07f) return rb::fail(e, RB_ERR_INVALID_CAMERA_DIRECTION, "Invalid camera direction");
    } else if (c->uniforms.change == RB_DELETE) {
        return rb::fail(e, RB_ERR_CANNOT_DELETE_NONEXISTENT, "Cannot delete none existent");
    }
    if (has_data(c->spheres)) {
        const rb_sphere* s = static_cast<const rb_sphere*>(c->spheres.ptr);
        for (size_t i = 0; i < c->spheres.count; ++i)
            if (s[i].radius <= 0.0f) return rb::fail(e, RB_ERR_INVALID_SPHERES, "Invalid Spheres");
    }
    if (has_data(c->uvs)) {
        if (c->uvs.count % 2 != 0) return rb::fail(e, RB_ERR_INVALID_UVS, "Invalid UVs");
    } else if (c->uvs.change == RB_DELETE) {
        return rb::fail(e, RB_ERR_UNSUPPORTED_DELETE, "not yet implemented: Implement UVs Deletion");
    }
    if (c->meshes.change == RB_DELETE)
        return rb::fail(e, RB_ERR_UNSUPPORTED_DELETE, "not yet implemented: Implement meshes Deletion");
    if (has_data(c->lights)) {
        const rb_point_light* l = static_cast<const rb_point_light*>(c->lights.ptr);
        for (size_t i = 0; i < c->lights.count; ++i)
            if (l[i].radius <= 0.0f) return rb::fail(e, RB_ERR_INVALID_LIGHTS, "Invalid Lights");
    } else if (c->lights.change == RB_DELETE) {
        return rb::fail(e, RB_ERR_UNSUPPORTED_DELETE, "not yet implemented: Implement lights Deletion");
    }
    if (c->textures.change == RB_DELETE)
        return rb::fail(e, RB_ERR_UNSUPPORTED_DELETE, "not yet implemented: Implement textures Deletion");
    return RB_OK;
}

struct StripeGeometry {
    uint32_t local = 0, padded = 0;
};
StripeGeometry stripe_geometry(const rb_options& opt, uint32_t h) {
    const uint32_t sc = opt.shard_count > 1 ? opt.shard_count : 1;
    const uint32_t sr = opt.stripe_rows ? opt.stripe_rows : rb::kDefaultStripeRows;
    StripeGeometry g{h, h};
    if (sc > 1) {
        const uint32_t stripes = (h + sr - 1) / sr;
        const uint32_t per_rank = (stripes + sc - 1) / sc;  // equal on every rank (padded)
        g.padded = per_rank * sr;
        uint32_t owned = 0;  // stripes this rank renders
        for (uint32_t s = opt.shard_rank; s < stripes; s += sc) owned++;
        g.local = owned * sr;  // the kernels additionally bound rows by global y < height
    }
    return g;
}

// grow_resolution -- buffers.rs:171-180 (+ the stripe geometry of the sharded case)
int resize_frame(rb_engine* e, uint32_t w, uint32_t h) {
    const StripeGeometry g = stripe_geometry(e->opt, h);
    const uint64_t px = static_cast<uint64_t>(w) * g.padded;
    if (px >= (1ull << 31)) return rb::fail(e, RB_ERR_INVALID_UNIFORMS, "frame of %u x %u pixels is too large", w, h);
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
    e->width = w;
    e->height = h;
    e->local_rows = g.local;
    e->padded_rows = g.padded;
    return RB_OK;
}

int upload_textures(rb_engine* e, const rb_field& f) {
    const rb_texture* t = static_cast<const rb_texture*>(f.ptr);
    std::vector<uint32_t> data;
    std::vector<rb_texture_info> info;
    uint32_t offset = 0;
    for (size_t i = 0; i < f.count; ++i) {  // process_textures, buffers.rs:151-168
        const size_t n = static_cast<size_t>(t[i].width) * t[i].height;
        info.push_back(rb_texture_info{offset, t[i].width, t[i].height, 0});
        data.insert(data.end(), t[i].rgba_data, t[i].rgba_data + n);
        offset += t[i].width * t[i].height;
    }
    int rc = rb::upload(e, e->tex_data, data.data(), data.size(), nullptr, true);
    if (rc) return rc;
    rc = rb::upload(e, e->tex_info, info.data(), info.size(), nullptr, true);
    if (rc) return rc;
    HIP_TRY(e, hipStreamSynchronize(e->stream));  // `data`/`info` are locals
    e->n_tex = static_cast<uint32_t>(f.count);
    return RB_OK;
}

int prep_materials(rb_engine* e, rb_material* first, size_t stride, size_t n) {
    if (!first || n == 0) return RB_OK;
    int rc = rb::launch_prep_materials(first, static_cast<uint32_t>(stride), static_cast<uint32_t>(n), e->stream);
    if (rc) return rb::fail(e, RB_ERR_DEVICE, "material prep launch failed: %s", hipGetErrorString(static_cast<hipError_t>(rc)));
    return RB_OK;
}

// What an update does with one non-uniform field.  `first` = the engine's first update
// (gpu_wrapper.rs:117-163: only Create is acted on); otherwise :196-294.
enum class Act { None, Take, Delete };
Act field_action(int idx, const rb_field& f, bool first) {
    const bool bvh_field = (idx >= 5 && idx <= 7);
    if (first) return f.change == RB_CREATE ? Act::Take : Act::None;
    if (f.change == RB_UPDATE) return Act::Take;
    if (f.change == RB_DELETE) return Act::Delete;
    if (f.change == RB_CREATE) return bvh_field ? Act::Take : Act::None;  // "Create not allowed after initialization" except BVH (:242-280)
    return Act::None;
}

int apply_field(rb_engine* e, int idx, const rb_field& f, bool first) {
    const Act act = field_action(idx, f, first);
    if (act == Act::None) return RB_OK;
    const bool del = act == Act::Delete;
    const void* src = del ? nullptr : f.ptr;
    const size_t n = del ? 0 : f.count;
    int rc = RB_OK;
    switch (idx) {
        case 1:
            rc = rb::upload(e, e->spheres, src, n, nullptr, true);
            e->n_spheres = static_cast<uint32_t>(n);
            if (!rc) rc = prep_materials(e, e->spheres.ptr ? &e->spheres.ptr->material : nullptr, sizeof(rb_sphere), n);
            if (!rc) rc = rb::build_sphere_bvh(e, static_cast<const rb_sphere*>(src), n);
            break;
        case 2: rc = rb::upload(e, e->uvs, src, n, nullptr, true); e->n_uvs = static_cast<uint32_t>(n); break;
        case 3:
            rc = rb::upload(e, e->meshes, src, n, nullptr, true);
            e->n_meshes = static_cast<uint32_t>(n);
            if (!rc) rc = prep_materials(e, e->meshes.ptr ? &e->meshes.ptr->material : nullptr, sizeof(rb_mesh), n);
            break;
        case 4:
            // delete_lights creates a 4-byte buffer (buffers.rs:389-391): arrayLength() == 0
            rc = rb::upload(e, e->lights, src, n, &e->n_lights, !del);
            if (del) e->n_lights = 0;
            if (!rc) rc = prep_materials(e, e->lights.ptr ? &e->lights.ptr->material : nullptr, sizeof(rb_point_light), e->n_lights);
            break;
        case 5:
            rc = rb::upload(e, e->nodes, src, n, nullptr, true);
            e->n_nodes = static_cast<uint32_t>(n);
            e->host_nodes.assign(static_cast<const rb_bvh_node*>(src), static_cast<const rb_bvh_node*>(src) + n);
            e->prep_dirty = true;
            e->tree = {n ? "caller" : "", 0.0f};
            break;
        case 6:
            rc = rb::upload(e, e->indices, src, n, &e->n_indices, true);
            e->prep_dirty = true;
            if (rb::mesh_walks(e->opt).host_mesh) {
                e->host_index_len = n;
                e->host_indices_stale = rb::host_copy_can_wait(e, n);
                if (e->host_indices_stale) std::vector<uint32_t>().swap(e->host_indices);
                else e->host_indices.assign(static_cast<const uint32_t*>(src), static_cast<const uint32_t*>(src) + n);
            }
            break;
        case 7:
            rc = rb::upload(e, e->tris, src, n, nullptr, true);
            e->n_tris = static_cast<uint32_t>(n);
            e->prep_dirty = true;
            if (rb::mesh_walks(e->opt).host_mesh) {
                e->host_tri_len = n;
                e->host_tris_stale = rb::host_copy_can_wait(e, n);
                if (e->host_tris_stale) std::vector<rb_gpu_triangle>().swap(e->host_tris);
                else e->host_tris.assign(static_cast<const rb_gpu_triangle*>(src), static_cast<const rb_gpu_triangle*>(src) + n);
            }
            break;
        case 8:
            if (del) { rb_field empty{RB_UPDATE, nullptr, 0}; rc = upload_textures(e, empty); }
            else rc = upload_textures(e, f);
            break;
        default: break;
    }
    return rc;
}

// Host-side checks that stand in for WGSL's robust buffer access: anything that would make a HIP kernel
// read out of bounds or loop forever is refused.  They run on the scene the update WOULD produce -- the
// incoming fields merged with the kept host copies -- before a single buffer is touched, so a refused
// rb_update leaves the previous scene live and renderable.
struct ScenePlan {
    uint32_t bvh_stack = 0, max_mesh_index = 0;
};
int validate_scene(rb_engine* e, const rb_config* cfg, bool first, ScenePlan& plan) {
    const Act a_nodes = field_action(5, cfg->bvh_nodes, first), a_idx = field_action(6, cfg->bvh_indices, first),
              a_tris = field_action(7, cfg->bvh_triangles, first), a_meshes = field_action(3, cfg->meshes, first);
    const bool take_uniforms = first ? (cfg->uniforms.change == RB_CREATE) : (cfg->uniforms.change == RB_UPDATE);
    // ---- the tree the kernels would walk
    const rb_bvh_node* nodes = e->host_nodes.data();
    uint32_t n_nodes = static_cast<uint32_t>(e->host_nodes.size());
    rb::TreeSkeleton own;   // RB_FLAG_BUILD_TREE: the tree the engine will build -- its shape follows from the triangle count
    const bool own_tree = rb::builds_tree(e);
    if (own_tree && (cfg->bvh_nodes.change != RB_KEEP || cfg->bvh_indices.change != RB_KEEP))
        return rb::fail(e, RB_ERR_INVALID_BVH, "the engine builds the tree itself (RB_FLAG_BUILD_TREE): bvh_nodes and bvh_indices must be Keep");
    if (own_tree && a_tris == Act::Take) {
        const rb_gpu_triangle* t = static_cast<const rb_gpu_triangle*>(cfg->bvh_triangles.ptr);
        if (cfg->bvh_triangles.count >= (1ull << 31)) return rb::fail(e, RB_ERR_INVALID_BVH, "too many triangles");
        const size_t bad = rb::first_non_finite(t, cfg->bvh_triangles.count);
        if (bad < cfg->bvh_triangles.count)
            return rb::fail(e, RB_ERR_INVALID_BVH, "triangle %zu has a non-finite vertex coordinate", bad);
        rb::bvh_skeleton(cfg->bvh_triangles.count, own);
        nodes = own.nodes.data();
        n_nodes = static_cast<uint32_t>(own.nodes.size());
    } else if (own_tree && a_tris == Act::Delete) {
        n_nodes = 0;
    } else if (a_nodes == Act::Take) {
        nodes = static_cast<const rb_bvh_node*>(cfg->bvh_nodes.ptr);
        if (cfg->bvh_nodes.count >= (1ull << 31)) return rb::fail(e, RB_ERR_INVALID_BVH, "too many BVH nodes");
        n_nodes = static_cast<uint32_t>(cfg->bvh_nodes.count);
    } else if (a_nodes == Act::Delete) {
        n_nodes = 0;
    }
    uint64_t index_len = e->n_indices;  // arrayLength(&bvh_indices): an empty vector still has one element
    if (a_idx == Act::Take) index_len = std::max<uint64_t>(cfg->bvh_indices.count, 1);
    else if (a_idx == Act::Delete) index_len = 1;
    if (own_tree && a_tris == Act::Take) index_len = std::max<uint64_t>(cfg->bvh_triangles.count, 1);
    else if (own_tree && a_tris == Act::Delete) index_len = 1;
    if (index_len >= (1ull << 31)) return rb::fail(e, RB_ERR_INVALID_BVH, "too many BVH indices");
    plan.bvh_stack = e->bvh_stack;
    if (n_nodes > 0) {
        std::string why;
        uint32_t depth = 0;
        if (!rb::bvh_validate(nodes, n_nodes, rb::kStackDepth, why, &depth)) return rb::fail(e, RB_ERR_INVALID_BVH, "%s", why.c_str());
        plan.bvh_stack = depth;
        for (uint32_t i = 0; i < n_nodes; ++i) {
            const rb_bvh_node& n = nodes[i];
            if (n.primitive_count > 0 && static_cast<uint64_t>(n.first_primitive) + n.primitive_count > index_len)
                return rb::fail(e, RB_ERR_INVALID_BVH, "leaf %u covers [%u, +%u) of %llu bvh_indices", i, n.first_primitive,
                            n.primitive_count, static_cast<unsigned long long>(index_len));
        }
    }
    // ---- every triangle's material must exist (shader.wgsl:370 reads meshes[tri.mesh_index])
    uint64_t n_tris = e->n_tris;
    plan.max_mesh_index = e->max_mesh_index;
    if (a_tris == Act::Take) {
        const rb_gpu_triangle* t = static_cast<const rb_gpu_triangle*>(cfg->bvh_triangles.ptr);
        uint32_t mx = 0;
        for (size_t i = 0; i < cfg->bvh_triangles.count; ++i) mx = std::max(mx, t[i].mesh_index);
        plan.max_mesh_index = mx;
        n_tris = cfg->bvh_triangles.count;
        if (n_tris >= (1ull << 31)) return rb::fail(e, RB_ERR_INVALID_BVH, "too many triangles");
    } else if (a_tris == Act::Delete) {
        n_tris = 0;
        plan.max_mesh_index = 0;
    }
    uint64_t n_meshes = e->n_meshes;
    if (a_meshes == Act::Take) n_meshes = cfg->meshes.count;
    const uint32_t color_hash = take_uniforms ? static_cast<const rb_uniforms*>(cfg->uniforms.ptr)->color_hash_enabled
                                              : e->uniforms.color_hash_enabled;
    if (n_tris > 0 && color_hash == 0 && plan.max_mesh_index >= n_meshes)
        return rb::fail(e, RB_ERR_INVALID_MESHES, "a triangle references mesh %u of %llu", plan.max_mesh_index,
                    static_cast<unsigned long long>(n_meshes));
    // ---- textures and the frame
    if (field_action(8, cfg->textures, first) == Act::Take) {
        const rb_texture* t = static_cast<const rb_texture*>(cfg->textures.ptr);
        for (size_t i = 0; i < cfg->textures.count; ++i) {
            if (t[i].width == 0 || t[i].height == 0) return rb::fail(e, RB_ERR_INVALID_TEXTURES, "texture %zu is empty", i);
            if (!t[i].rgba_data) return rb::fail(e, RB_ERR_INVALID_TEXTURES, "texture %zu has no data", i);
        }
    }
    if (take_uniforms) {
        const rb_uniforms* u = static_cast<const rb_uniforms*>(cfg->uniforms.ptr);
        const uint64_t px = static_cast<uint64_t>(u->width) * stripe_geometry(e->opt, u->height).padded;
        if (px >= (1ull << 31)) return rb::fail(e, RB_ERR_INVALID_UNIFORMS, "frame of %u x %u pixels is too large", u->width, u->height);
    }
    return RB_OK;
}

// update_uniforms count patch-up -- gpu_wrapper.rs:475-495: Create/Update overwrite the count with the
// vector length, Delete zeroes it, Keep leaves the caller's value (clamped to the buffer here so that a
// stale count cannot read out of bounds; the WGSL relies on robust buffer access for that).
uint32_t patch_count(uint32_t change, uint32_t given, uint32_t len) {
    if (change == RB_CREATE || change == RB_UPDATE) return len;
    if (change == RB_DELETE) return 0u;
    return std::min(given, len);
}

int ensure_prepared(rb_engine* e) {
    // shader.wgsl:336 skips triangle ids >= uniforms.bvh_triangle_count: the prepared triangles carry that
    // guard as their `valid` word, so they depend on the (patched) count as well as on the buffers
    const uint32_t tri_count = patch_count(e->last_change_tris, e->uniforms.bvh_triangle_count, e->n_tris);
    if (!e->prep_dirty && e->prep_tri_count == tri_count) return RB_OK;
    const uint32_t len = e->n_indices;  // arrayLength(&bvh_indices) >= 1
    HIP_TRY(e, e->ptris.resize(len));
    HIP_TRY(e, e->pshade.resize(len));
    int rc = rb::launch_prep_tris(e->tris.ptr, tri_count, e->indices.ptr, len, e->ptris.ptr, e->pshade.ptr, e->stream);
    if (rc) return rb::fail(e, RB_ERR_DEVICE, "prep kernel launch failed: %s", hipGetErrorString(static_cast<hipError_t>(rc)));
    e->prep_dirty = false;
    e->prep_tri_count = tri_count;
    // ---- the mesh walk's tree (rb_accel.cpp): the chunked walk's if wanted, else the library's own if wanted
    e->chunk.rec = e->own.rec = {};
    rc = rb::build_chunk_tree(e, tri_count);
    return (rc || e->chunk.rec.built()) ? rc : rb::build_own_tree(e, tri_count);
}

rb::KParams make_params(rb_engine* e, uint32_t first_pass, uint32_t n_passes, int src, int dst) {
    rb::KParams p{};
    p.u = e->uniforms;
    p.u.spheres_count = patch_count(e->last_change_spheres, e->uniforms.spheres_count, e->n_spheres);
    p.u.bvh_node_count = patch_count(e->last_change_nodes, e->uniforms.bvh_node_count, e->n_nodes);
    p.u.bvh_triangle_count = patch_count(e->last_change_tris, e->uniforms.bvh_triangle_count, e->n_tris);
    p.spheres = e->spheres.ptr;
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
    p.n_lights = e->n_lights;
    p.n_meshes = e->n_meshes;
    p.index_len = e->n_indices;
    p.n_uvs = e->n_uvs;
    p.n_tex = e->n_tex;
    p.first_pass = first_pass;
    p.n_passes = n_passes;
    p.samples_per_pass = e->prh.samples_per_pass;
    p.shard_rank = e->opt.shard_rank;
    p.shard_count = e->opt.shard_count > 1 ? e->opt.shard_count : 1;
    p.stripe_rows = e->opt.stripe_rows ? e->opt.stripe_rows : rb::kDefaultStripeRows;
    p.local_rows = e->local_rows;
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
    return p;
}

int require_ready(rb_engine* e) {
    if (!e->initialized) return rb::fail(e, RB_ERR_NOT_INITIALIZED, "engine has not received its first update");
    if (!e->scene_valid) return rb::fail(e, RB_ERR_DEVICE, "the last update failed half-way on the device; send the scene again");
    if (!e->have_uniforms) return rb::fail(e, RB_ERR_UNIFORMS_NOT_INITIALIZED, "Uniforms must be initialized");
    return RB_OK;
}

int clear_accum(rb_engine* e) {
    const size_t px = static_cast<size_t>(e->width) * e->padded_rows;
    e->spec_valid = false;
    if (px) HIP_TRY(e, hipMemsetAsync(e->slot[e->cur].accum.ptr, 0, px * 16, e->stream));
    return RB_OK;
}

int accumulate_timing(rb_engine* e) {
    float ms = 0.0f;
    if (e->last_launches > 0) {
        HIP_TRY(e, hipEventSynchronize(e->ev_end));
        HIP_TRY(e, hipEventElapsedTime(&ms, e->ev_begin, e->ev_end));
    }
    e->last_dispatch_ms = ms;
    if (e->timing_pending) {
        e->stats.kernel_ms += ms;
        for (uint32_t i = 0; i + 3 <= e->ev_used; i += 3) {
            float t = 0.0f, a = 0.0f;
            HIP_TRY(e, hipEventElapsedTime(&t, e->ev_pool[i], e->ev_pool[i + 1]));
            HIP_TRY(e, hipEventElapsedTime(&a, e->ev_pool[i + 1], e->ev_pool[i + 2]));
            e->stats.trace_ms += t;
            e->stats.accumulate_ms += a;
        }
        e->timing_pending = false;
    }
    return RB_OK;
}

// Colour-buffer budget of the stream kernels (one float4 per (pixel, sample) of a launch chunk): the caller's
// figure, else 4 GiB but never more than half of what the device has free right now -- eight launches per C2
// frame instead of one cost 0.4 %, and a library that sits behind a GUI should not take 34 GB for a 1080p frame.
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

// The stream kernels' colour buffer for a group of n_passes passes, and the passes per launch it allows: one float4 per
// (pixel, sample) of a launch chunk.  Keeps the item count below 2^31 and, unless the caller fixed the chunk, the buffer
// within the budget; if the device cannot give even that, halves.  Allocates (lazily: the first dispatch, or rb_reserve).
int reserve_colors(rb_engine* e, uint32_t n_passes, uint32_t* chunk_out) {
    const uint32_t kernel = rb::kernel_of(e->opt);
    uint32_t chunk = e->opt.passes_per_launch ? e->opt.passes_per_launch : n_passes;
    if (kernel == RB_KERNEL_STREAM && n_passes != 0 && e->width != 0 && e->local_rows != 0) {
        const uint64_t tiles = static_cast<uint64_t>((e->width + 7) / 8) * ((e->local_rows + 7) / 8);
        const uint64_t per_pass = tiles * 64ull * e->prh.samples_per_pass;  // items per pass
        const uint64_t budget_items = color_budget_bytes(e) / 16ull;
        uint64_t max_chunk = std::min<uint64_t>((1ull << 31) / std::max<uint64_t>(per_pass, 1) , 0xFFFFFFFFull);
        if (!e->opt.passes_per_launch) max_chunk = std::min(max_chunk, std::max<uint64_t>(budget_items / std::max<uint64_t>(per_pass, 1), 1));
        if (max_chunk == 0) return rb::fail(e, RB_ERR_INVALID_UNIFORMS, "frame too large for one launch");
        chunk = static_cast<uint32_t>(std::min<uint64_t>(chunk, max_chunk));
        for (;;) {
            const hipError_t st = e->colors.reserve(per_pass * chunk * 4);
            if (st == hipSuccess) break;
            (void)hipGetLastError();  // clear the sticky out-of-memory status
            if (st != hipErrorOutOfMemory || chunk == 1)
                return rb::fail(e, RB_ERR_DEVICE, "colour buffer of %llu bytes: %s", static_cast<unsigned long long>(per_pass * chunk * 16ull),
                            hipGetErrorString(st));
            chunk = (chunk + 1) / 2;
        }
    }
    *chunk_out = chunk;
    return RB_OK;
}

// dispatch_compute_progressive without the host sync -- gpu_wrapper.rs:365-400: passes
// [first_pass, first_pass + n_passes) on top of slot `src`, into slot `dst` (the same slot, or the other one
// when the iterator runs a pass ahead).
int dispatch(rb_engine* e, uint32_t first_pass, uint32_t n_passes, int src, int dst) {
    int rc = ensure_prepared(e);
    if (rc) return rc;
    if (n_passes == 0 || e->width == 0 || e->local_rows == 0) {
        e->last_launches = 0;
        return RB_OK;
    }
    if (e->timing_pending) {  // fold the previous group's events before they are recorded again
        rc = accumulate_timing(e);
        if (rc) return rc;
    }
    const uint32_t kernel = rb::kernel_of(e->opt);
    const bool stats = (e->opt.flags & RB_FLAG_STATS) != 0;
    uint32_t chunk = 0;
    rc = reserve_colors(e, n_passes, &chunk);
    if (rc) return rc;
    HIP_TRY(e, hipEventRecord(e->ev_begin, e->stream));
    uint32_t launches = 0;
    e->ev_used = 0;
    for (uint32_t done = 0; done < n_passes;) {
        const uint32_t n = std::min(chunk, n_passes - done);
        // the first chunk resumes `src`; later chunks of the same group continue in `dst`
        rb::KParams p = make_params(e, first_pass + done, n, done == 0 ? src : dst, dst);
        if (!e->stack_depth_covers) return rb::fail(e, RB_ERR_DEVICE, "internal: a traversal is deeper than its LDS stack column (%u entries)", p.stack_depth);
        rb::LaunchInfo li{};
        // per-chunk timing events (first 256 chunks of a group; later ones only count in the total)
        hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
        if (e->ev_used + 3 <= 768) {
            while (e->ev_pool.size() < e->ev_used + 3) {
                hipEvent_t x;
                HIP_TRY(e, hipEventCreate(&x));
                e->ev_pool.push_back(x);
            }
            for (int i = 0; i < 3; ++i) ev[i] = e->ev_pool[e->ev_used + i];
            e->ev_used += 3;
            HIP_TRY(e, hipEventRecord(ev[0], e->stream));
        }
        rc = rb::launch_render(p, kernel, stats, e->stream, &li, ev[1]);
        if (rc) return rb::fail(e, RB_ERR_DEVICE, "render kernel launch failed: %s", hipGetErrorString(static_cast<hipError_t>(rc)));
        if (ev[2]) {
            if (kernel != RB_KERNEL_STREAM) HIP_TRY(e, hipEventRecord(ev[1], e->stream));
            HIP_TRY(e, hipEventRecord(ev[2], e->stream));
        }
        if (li.kernel_name) e->last_kernel_name = li.kernel_name;
        done += n;
        launches++;
    }
    HIP_TRY(e, hipEventRecord(e->ev_end, e->stream));
    HIP_TRY(e, hipEventRecord(e->slot[dst].done, e->stream));
    e->last_launches = launches;
    e->timing_pending = true;
    e->stats.launches += launches;
    return RB_OK;
}

// Copies the committed frame's RGBA8 rows (local stripe order when sharded) to caller memory: the host waits
// for the launches that produced the slot, then a blocking copy.  The engine's stream is non-blocking, so a
// pass the iterator has already started on the OTHER slot keeps running underneath this copy.
int read_slot_rgba(rb_engine* e, int slot, uint8_t* out) {
    if (!out) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "rgba_out is NULL");
    const uint32_t sc = e->opt.shard_count > 1 ? e->opt.shard_count : 1;
    const size_t bytes = static_cast<size_t>(e->width) * 4 * (sc == 1 ? e->height : e->padded_rows);
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
    int rc = check_fields(e, cfg);
    if (rc) return rc;
    const bool first = !e->initialized;
    rc = first ? validate_init(e, cfg) : validate(e, cfg);
    if (rc) return rc;
    ScenePlan plan;
    rc = validate_scene(e, cfg, first, plan);
    if (rc) return rc;   // nothing has been touched: the previous scene stays live

    // ---- from here on the buffers change; a device failure half-way leaves the engine refusing to render
    e->scene_valid = false;
    e->spec_valid = false;
    e->color_budget = 0;
    e->dn_guides_valid = false;   // the denoiser's guides are this scene's and this camera's
    // uniforms (gpu_wrapper.rs:122-136 / :165-192)
    const bool take_uniforms = first ? (cfg->uniforms.change == RB_CREATE) : (cfg->uniforms.change == RB_UPDATE);
    if (take_uniforms) {
        const rb_uniforms* u = static_cast<const rb_uniforms*>(cfg->uniforms.ptr);
        if (u->width != e->width || u->height != e->height || e->slot[0].accum.ptr == nullptr) {
            rc = resize_frame(e, u->width, u->height);
            if (rc) return rc;
        }
        e->uniforms = *u;
        e->prh.total_samples = u->total_samples;  // ProgressiveRenderHelper::update (:47-52)
        e->prh.total_passes = (u->total_samples + e->prh.samples_per_pass - 1) / e->prh.samples_per_pass;
    }
    // self.rc = new_rc (:298): width()/height()/update_uniforms panic unless the *latest*
    // config carried Create/Update uniforms (:303-329,470-473).
    e->have_uniforms = has_data(cfg->uniforms);

    for (int i = 1; i < 9; ++i) {
        rc = apply_field(e, i, *field_at(cfg, i), first);
        if (rc) return rc;
    }
    if (rb::builds_tree(e)) {   // the tree follows the triangles field (RB_FLAG_BUILD_TREE)
        const Act a_tris = field_action(7, cfg->bvh_triangles, first);
        if (a_tris != Act::None) {
            rc = rb::build_engine_tree(e, static_cast<const rb_gpu_triangle*>(a_tris == Act::Take ? cfg->bvh_triangles.ptr : nullptr),
                                   a_tris == Act::Take ? cfg->bvh_triangles.count : 0);
            if (rc) return rc;
        }
    }
    e->last_change_spheres = cfg->spheres.change;
    e->last_change_nodes = rb::builds_tree(e) ? cfg->bvh_triangles.change : cfg->bvh_nodes.change;
    e->last_change_tris = cfg->bvh_triangles.change;
    e->bvh_stack = plan.bvh_stack;
    e->max_mesh_index = plan.max_mesh_index;
    e->initialized = true;
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
        if (rb::gather_process(e->net, e->slot[e->cur].rgba.ptr, e->width, e->height, e->padded_rows,
                               e->opt.stripe_rows ? e->opt.stripe_rows : rb::kDefaultStripeRows, e->copy_stream, e->slot[e->cur].done,
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
        const size_t px = static_cast<size_t>(e->width) * e->padded_rows;
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
        if (rb::gather_process(e->net, e->slot[e->cur].rgba.ptr, e->width, e->height, e->padded_rows,
                               e->opt.stripe_rows ? e->opt.stripe_rows : rb::kDefaultStripeRows, e->copy_stream, e->slot[e->cur].done,
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
    // RB_REFERENCE_WALK=1 in the environment: every engine of this process walks meshes exactly as shader.wgsl:282-392 does,
    // whatever the host program's flags say -- the escape hatch from the culled walks (whose exactness is derived and fuzzed,
    // DESIGN.md section 4.2) that needs no rebuild of the host
    if (const char* rw = std::getenv("RB_REFERENCE_WALK"); rw && rw[0] == '1')
        e->opt.flags = (e->opt.flags & ~(rb::kOwnTreeFlags | RB_FLAG_DEVICE_LBVH | RB_FLAG_CHUNK_WALK | RB_FLAG_SKIP_NEAR_DEGENERATE)) |
                       RB_FLAG_REFERENCE_WALK;
    auto bail = [&](const char* what, hipError_t st) -> rb_engine* {
        rb::fail(nullptr, RB_ERR_DEVICE, "%s failed: %s", what, hipGetErrorString(st));
        rb_destroy(e);
        return nullptr;
    };
    hipError_t st;
    if ((st = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking)) != hipSuccess) return bail("hipStreamCreate", st);
    if ((st = hipStreamCreateWithFlags(&e->copy_stream, hipStreamNonBlocking)) != hipSuccess) return bail("hipStreamCreate", st);
    if ((st = hipEventCreate(&e->ev_begin)) != hipSuccess) return bail("hipEventCreate", st);
    if ((st = hipEventCreate(&e->ev_end)) != hipSuccess) return bail("hipEventCreate", st);
    for (rb::FrameSlot& s : e->slot)
        if ((st = hipEventCreateWithFlags(&s.done, hipEventDisableTiming)) != hipSuccess) return bail("hipEventCreate", st);
    if ((st = e->counters.resize(rb::C_COUNT)) != hipSuccess) return bail("hipMalloc(counters)", st);
    if ((st = e->queue.resize(rb::kQueueWords)) != hipSuccess) return bail("hipMalloc(queue)", st);
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
    if (!cfg) { rb::fail(nullptr, RB_ERR_NULL_ARGUMENT, "config is NULL"); return false; }
    if (check_fields(nullptr, cfg)) return false;
    // GpuBuffers::new panics unless these are Create (buffers.rs:74-97)
    if (validate_init(nullptr, cfg)) return false;
    return true;
}

rb_engine* create_impl(const rb_config* cfg, const rb_options* opt_in) {
    if (!check_create(cfg)) return nullptr;
    rb_options opt{};
    opt.device = -1;
    if (opt_in) opt = *opt_in;
    return create_single(cfg, opt);
}

// ------------------------------------------------------------------ several devices, one handle ----
void copy_error(rb_engine* g, const rb_engine* part) {
    std::string msg;
    {
        std::lock_guard<std::mutex> l(part->err_mu);
        msg = part->error;
    }
    std::lock_guard<std::mutex> l(g->err_mu);
    g->error = "device " + std::to_string(part->device) + ": " + msg;
}

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
    g->width = p0->width;
    g->height = p0->height;
    g->have_uniforms = p0->have_uniforms;
    g->initialized = p0->initialized;
    g->prh = p0->prh;
    return RB_OK;
}

// the one exchange step: every part's RGBA8 stripes to the root device, de-interleaved there, then read back
int group_deliver(rb_engine* g, uint8_t* rgba_out, bool fold_timing) {
    std::vector<rb::GatherSource> src;
    for (auto& p : g->parts) src.push_back(rb::GatherSource{p->device, p->copy_stream, p->slot[p->cur].done, p->slot[p->cur].rgba.ptr});
    rb_engine* p0 = g->parts[0].get();
    const uint32_t sr = p0->opt.stripe_rows ? p0->opt.stripe_rows : rb::kDefaultStripeRows;
    std::string why;
    if (rb::gather_group(g->net, src, p0->width, p0->height, p0->padded_rows, sr, rgba_out, why))
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

// ------------------------------------------------------------------ closest-hit queries ----
// (rb_abi.h)  A query reads the scene and writes its own scratch: it is queued on the engine's stream
// behind whatever runs there -- a pass the iterator has started ahead included, which stays valid -- and uses events of its
// own, so neither the work counters nor the timing of a launch group move.
bool page_locked(const void* p) {
    hipPointerAttribute_t attr{};
    if (p && hipPointerGetAttributes(&attr, p) == hipSuccess && attr.type == hipMemoryTypeHost) return true;
    (void)hipGetLastError();   // an unregistered pointer makes the query fail: that is the ordinary case
    return false;
}

// device -> caller memory behind the stream's work: a DMA into page-locked memory, a blocking copy otherwise
int query_copy_out(rb_engine* e, void* dst, const void* src, size_t bytes, bool pinned) {
    if (pinned) {
        HIP_TRY(e, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, e->stream));
        return RB_OK;
    }
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    HIP_TRY(e, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return RB_OK;
}

// the scene as a query's kernels see it, and the query's two events
int query_params(rb_engine* e, rb::KParams* p) {
    int rc = require_ready(e);
    if (!rc) rc = ensure_prepared(e);
    if (rc) return rc;
    *p = make_params(e, 0, 0, e->cur, e->cur);
    if (!e->stack_depth_covers) return rb::fail(e, RB_ERR_DEVICE, "internal: a traversal is deeper than its LDS stack column (%u entries)", p->stack_depth);
    for (hipEvent_t& x : e->ev_q)
        if (!x) HIP_TRY(e, hipEventCreate(&x));
    e->query_ms_pending = false;
    return RB_OK;
}

int query_begin(rb_engine* e, rb::KParams* p, size_t records, bool rays, bool surf) {
    const int rc = query_params(e, p);
    if (rc) return rc;
    if (rays) HIP_TRY(e, e->q_rays.reserve(records));
    HIP_TRY(e, e->q_hits.reserve(records));
    if (surf) HIP_TRY(e, e->q_surf.reserve(records));
    e->last_query_ms = 0.0f;
    return RB_OK;
}

// one piece: launch between the query's two events, copy the records out, fold the kernel time
int query_piece(rb_engine* e, const rb::KParams& p, rb::QueryArgs q, size_t records, rb_hit* hits_out, rb_surface* surf_out,
                bool hits_pinned, bool surf_pinned) {
    q.hits = e->q_hits.ptr;
    q.surf = surf_out ? e->q_surf.ptr : nullptr;
    rb::LaunchInfo li{};
    HIP_TRY(e, hipEventRecord(e->ev_q[0], e->stream));
    const int st = rb::launch_query(p, q, e->stream, &li);
    if (st) return rb::fail(e, RB_ERR_DEVICE, "query kernel launch failed: %s", hipGetErrorString(static_cast<hipError_t>(st)));
    HIP_TRY(e, hipEventRecord(e->ev_q[1], e->stream));
    if (li.kernel_name) e->last_query_kernel_name = li.kernel_name;
    int rc = query_copy_out(e, hits_out, e->q_hits.ptr, records * sizeof(rb_hit), hits_pinned);
    if (!rc && surf_out) rc = query_copy_out(e, surf_out, e->q_surf.ptr, records * sizeof(rb_surface), surf_pinned);
    if (rc) return rc;
    HIP_TRY(e, hipStreamSynchronize(e->stream));   // the scratch is the next piece's
    float ms = 0.0f;
    HIP_TRY(e, hipEventElapsedTime(&ms, e->ev_q[0], e->ev_q[1]));
    e->last_query_ms += ms;
    return RB_OK;
}

int cast_rays_locked(rb_engine* e, const rb_ray* rays, size_t n, rb_hit* hits_out, rb_surface* surf_out) {
    rb::KParams p{};
    const size_t piece = std::min<size_t>(n, rb::kQueryPiece);
    int rc = query_begin(e, &p, piece, true, surf_out != nullptr);
    if (rc || n == 0) return rc;
    const bool hits_pinned = page_locked(hits_out), surf_pinned = page_locked(surf_out);
    for (size_t done = 0; done < n; done += piece) {
        const size_t m = std::min(piece, n - done);
        // (from pageable memory the runtime stages the copy and returns when the source may be reused)
        HIP_TRY(e, hipMemcpyAsync(e->q_rays.ptr, rays + done, m * sizeof(rb_ray), hipMemcpyHostToDevice, e->stream));
        rb::QueryArgs q{};
        q.rays = e->q_rays.ptr;
        q.n = static_cast<uint32_t>(m);
        rc = query_piece(e, p, q, m, hits_out + done, surf_out ? surf_out + done : nullptr, hits_pinned, surf_pinned);
        if (rc) return rc;
    }
    return RB_OK;
}

// the pixel centres of rows [0, rows) x the whole width (global = image rows, else this shard's local rows), or of one pixel
int pixel_hits_locked(rb_engine* e, uint32_t x0, uint32_t y0, uint32_t w, uint32_t rows, bool global, rb_hit* hits_out, rb_surface* surf_out) {
    rb::KParams p{};
    const uint32_t piece_rows = w == 0 ? 8u : std::max<uint32_t>(8u, (rb::kQueryPiece / w) & ~7u);   // whole 8-row tiles
    int rc = query_begin(e, &p, static_cast<size_t>(std::min(piece_rows, rows)) * w, false, surf_out != nullptr);
    if (rc || w == 0 || rows == 0) return rc;
    const bool hits_pinned = page_locked(hits_out), surf_pinned = page_locked(surf_out);
    for (uint32_t r0 = 0; r0 < rows; r0 += piece_rows) {
        const uint32_t h = std::min(piece_rows, rows - r0);
        rb::QueryArgs q{};
        q.win_x = x0;
        q.win_y = y0 + r0;
        q.win_w = w;
        q.win_h = h;
        q.win_global = global ? 1u : 0u;
        const size_t off = static_cast<size_t>(r0) * w;
        rc = query_piece(e, p, q, static_cast<size_t>(h) * w, hits_out + off, surf_out ? surf_out + off : nullptr, hits_pinned, surf_pinned);
        if (rc) return rc;
    }
    return RB_OK;
}

// ---- any-hit occlusion and the device forms (rb_abi.h)
int occluded_locked(rb_engine* e, const rb_ray* rays, const float* tmax, size_t n, uint32_t mask, uint8_t* out) {
    rb::KParams p{};
    int rc = query_params(e, &p);
    e->last_query_ms = 0.0f;
    if (rc || n == 0) return rc;
    const size_t piece = std::min<size_t>(n, rb::kQueryPiece);
    HIP_TRY(e, e->q_rays.reserve(piece));
    if (tmax) HIP_TRY(e, e->q_tmax.reserve(piece));
    HIP_TRY(e, e->q_occl.reserve(piece));
    const bool pinned = page_locked(out);
    for (size_t done = 0; done < n; done += piece) {
        const size_t m = std::min(piece, n - done);
        HIP_TRY(e, hipMemcpyAsync(e->q_rays.ptr, rays + done, m * sizeof(rb_ray), hipMemcpyHostToDevice, e->stream));
        if (tmax) HIP_TRY(e, hipMemcpyAsync(e->q_tmax.ptr, tmax + done, m * sizeof(float), hipMemcpyHostToDevice, e->stream));
        rb::OcclArgs a{};
        a.q.rays = e->q_rays.ptr;
        a.q.n = static_cast<uint32_t>(m);
        a.tmax = tmax ? e->q_tmax.ptr : nullptr;
        a.out = e->q_occl.ptr;
        a.mask = mask;
        rb::LaunchInfo li{};
        HIP_TRY(e, hipEventRecord(e->ev_q[0], e->stream));
        const int st = rb::launch_occluded(p, a, e->stream, &li);
        if (st) return rb::fail(e, RB_ERR_DEVICE, "occlusion kernel launch failed: %s", hipGetErrorString(static_cast<hipError_t>(st)));
        HIP_TRY(e, hipEventRecord(e->ev_q[1], e->stream));
        if (li.kernel_name) e->last_query_kernel_name = li.kernel_name;
        rc = query_copy_out(e, out + done, e->q_occl.ptr, m, pinned);
        if (rc) return rc;
        HIP_TRY(e, hipStreamSynchronize(e->stream));   // the scratch is the next piece's
        float ms = 0.0f;
        HIP_TRY(e, hipEventElapsedTime(&ms, e->ev_q[0], e->ev_q[1]));
        e->last_query_ms += ms;
    }
    return RB_OK;
}

// `bytes` of device memory of the engine's device at p, aligned to `align`?
int device_range(rb_engine* e, const void* p, size_t bytes, size_t align, const char* what) {
    hipPointerAttribute_t attr{};
    const hipError_t st = hipPointerGetAttributes(&attr, p);
    if (st != hipSuccess) (void)hipGetLastError();   // a pointer the runtime does not know: pageable host memory
    if (st != hipSuccess || attr.type != hipMemoryTypeDevice || attr.device != e->device)
        return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s is not device memory of device %d", what, e->device);
    if (reinterpret_cast<uintptr_t>(p) % align != 0u) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s is not %zu-byte aligned", what, align);
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void*>(p)) != hipSuccess) {
        (void)hipGetLastError();
        return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: its allocation is unknown to the runtime", what);
    }
    const size_t off = static_cast<size_t>(static_cast<const char*>(p) - static_cast<const char*>(base));
    if (off > size || bytes > size - off) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: its allocation ends before %zu bytes", what, bytes);
    return RB_OK;
}

// queue one launch between the query's events on the caller's buffers; nothing is waited for
template <class Launch>
int device_query_locked(rb_engine* e, Launch&& launch) {
    rb::KParams p{};
    const int rc = query_params(e, &p);
    e->last_query_ms = 0.0f;
    if (rc) return rc;
    rb::LaunchInfo li{};
    HIP_TRY(e, hipEventRecord(e->ev_q[0], e->stream));
    const int st = launch(p, &li);
    if (st) return rb::fail(e, RB_ERR_DEVICE, "query kernel launch failed: %s", hipGetErrorString(static_cast<hipError_t>(st)));
    HIP_TRY(e, hipEventRecord(e->ev_q[1], e->stream));
    if (li.kernel_name) e->last_query_kernel_name = li.kernel_name;
    e->query_ms_pending = true;   // rb_last_query_ms reads the events when it is asked
    return RB_OK;
}

int occluded_device_locked(rb_engine* e, const rb_ray* d_rays, const float* d_tmax, size_t n, uint32_t mask, uint8_t* d_out) {
    int rc = device_range(e, d_rays, n * sizeof(rb_ray), 16, "d_rays");
    if (!rc && d_tmax) rc = device_range(e, d_tmax, n * sizeof(float), 4, "d_tmax");
    if (!rc) rc = device_range(e, d_out, n, 1, "d_out");
    if (rc) return rc;
    return device_query_locked(e, [&](const rb::KParams& p, rb::LaunchInfo* li) {
        rb::OcclArgs a{};
        a.q.rays = d_rays;
        a.q.n = static_cast<uint32_t>(n);
        a.tmax = d_tmax;
        a.out = d_out;
        a.mask = mask;
        return rb::launch_occluded(p, a, e->stream, li);
    });
}

int cast_rays_device_locked(rb_engine* e, const rb_ray* d_rays, size_t n, rb_hit* d_hits, rb_surface* d_surf) {
    int rc = device_range(e, d_rays, n * sizeof(rb_ray), 16, "d_rays");
    if (!rc) rc = device_range(e, d_hits, n * sizeof(rb_hit), 16, "d_hits");
    if (!rc && d_surf) rc = device_range(e, d_surf, n * sizeof(rb_surface), 16, "d_surf");
    if (rc) return rc;
    return device_query_locked(e, [&](const rb::KParams& p, rb::LaunchInfo* li) {
        rb::QueryArgs q{};
        q.rays = d_rays;
        q.n = static_cast<uint32_t>(n);
        q.hits = d_hits;
        q.surf = d_surf;
        return rb::launch_query(p, q, e->stream, li);
    });
}

// ---- path-traced radiance along given rays (rb_abi.h)
// rays per piece: whole blocks of 64 rays, never a part of one ray's samples (samples <= 65536: at least one block)
size_t trace_piece_rays(uint32_t samples) { return std::max<size_t>((RB_TRACE_PIECE_ITEMS / samples) & ~size_t(63), 64); }

// the scratch of one piece: colours and the queue word
int trace_scratch(rb_engine* e, size_t piece, uint32_t samples) {
    HIP_TRY(e, e->rad_colors.reserve(((piece + 63) / 64) * 64 * samples * 4));
    HIP_TRY(e, e->rad_queue.reserve(16));
    return RB_OK;
}

rb::RadArgs trace_args(rb_engine* e, const rb_ray* rays, const uint32_t* seeds, rb_radiance* out, size_t done, size_t m,
                       uint32_t first_sample, uint32_t samples) {
    rb::RadArgs a{};
    a.rays = rays;
    a.seeds = seeds;
    a.colors = e->rad_colors.ptr;
    a.out = out;
    a.queue = e->rad_queue.ptr;
    a.n = static_cast<uint32_t>(m);
    a.seed_base = static_cast<uint32_t>(done);
    a.first_sample = first_sample;
    a.samples = samples;
    return a;
}

int trace_rays_locked(rb_engine* e, const rb_ray* rays, const uint32_t* seeds, size_t n, uint32_t first_sample, uint32_t samples,
                      rb_radiance* out) {
    rb::KParams p{};
    int rc = query_params(e, &p);
    e->last_query_ms = 0.0f;
    if (rc || n == 0) return rc;
    const size_t piece = std::min(n, trace_piece_rays(samples));
    rc = trace_scratch(e, piece, samples);
    if (rc) return rc;
    HIP_TRY(e, e->q_rays.reserve(piece));
    if (seeds) HIP_TRY(e, e->rad_seeds.reserve(piece));
    HIP_TRY(e, e->rad_out.reserve(piece));
    const bool pinned = page_locked(out);
    for (size_t done = 0; done < n; done += piece) {
        const size_t m = std::min(piece, n - done);
        HIP_TRY(e, hipMemcpyAsync(e->q_rays.ptr, rays + done, m * sizeof(rb_ray), hipMemcpyHostToDevice, e->stream));
        if (seeds) HIP_TRY(e, hipMemcpyAsync(e->rad_seeds.ptr, seeds + done, m * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
        const rb::RadArgs a = trace_args(e, e->q_rays.ptr, seeds ? e->rad_seeds.ptr : nullptr, e->rad_out.ptr, done, m, first_sample, samples);
        rb::LaunchInfo li{};
        HIP_TRY(e, hipEventRecord(e->ev_q[0], e->stream));
        const int st = rb::launch_radiance(p, a, e->stream, &li);
        if (st) return rb::fail(e, RB_ERR_DEVICE, "radiance kernel launch failed: %s", hipGetErrorString(static_cast<hipError_t>(st)));
        HIP_TRY(e, hipEventRecord(e->ev_q[1], e->stream));
        if (li.kernel_name) e->last_query_kernel_name = li.kernel_name;
        rc = query_copy_out(e, out + done, e->rad_out.ptr, m * sizeof(rb_radiance), pinned);
        if (rc) return rc;
        HIP_TRY(e, hipStreamSynchronize(e->stream));   // the scratch is the next piece's
        float ms = 0.0f;
        HIP_TRY(e, hipEventElapsedTime(&ms, e->ev_q[0], e->ev_q[1]));
        e->last_query_ms += ms;
    }
    return RB_OK;
}

// every piece queued between the query's two events on the caller's buffers (the pieces share the colour scratch in stream
// order); nothing is waited for
int trace_rays_device_locked(rb_engine* e, const rb_ray* d_rays, const uint32_t* d_seeds, size_t n, uint32_t first_sample,
                             uint32_t samples, rb_radiance* d_out) {
    int rc = device_range(e, d_rays, n * sizeof(rb_ray), 16, "d_rays");
    if (!rc && d_seeds) rc = device_range(e, d_seeds, n * sizeof(uint32_t), 4, "d_seeds");
    if (!rc) rc = device_range(e, d_out, n * sizeof(rb_radiance), 16, "d_out");
    if (rc) return rc;
    const size_t piece = std::min(n, trace_piece_rays(samples));
    return device_query_locked(e, [&](const rb::KParams& p, rb::LaunchInfo* li) {
        if (trace_scratch(e, piece, samples)) return static_cast<int>(hipErrorOutOfMemory);
        for (size_t done = 0; done < n; done += piece) {
            const size_t m = std::min(piece, n - done);
            const rb::RadArgs a = trace_args(e, d_rays + done, d_seeds ? d_seeds + done : nullptr, d_out + done, done, m, first_sample, samples);
            const int st = rb::launch_radiance(p, a, e->stream, li);
            if (st) return st;
        }
        return 0;
    });
}

// ---- camera rays made on the device (rb_abi.h)
// pixels per piece: whole blocks of 64 pixels, never a part of one pixel's samples (samples <= 65536: at least one block)
size_t camera_piece_pixels(uint32_t samples) { return std::max<size_t>((RB_CAMERA_PIECE_ITEMS / samples) & ~size_t(63), 64); }

// the scratch of one piece: a record and a colour per item, the queue word
int camera_scratch(rb_engine* e, size_t piece, uint32_t samples) {
    const size_t items = ((piece + 63) / 64) * 64 * samples;
    HIP_TRY(e, e->q_rays.reserve(items));
    HIP_TRY(e, e->rad_colors.reserve(items * 4));
    HIP_TRY(e, e->rad_queue.reserve(16));
    return RB_OK;
}

// one piece, queued: the generator into the record scratch, the k_cam kernel of the scene's walk over it, the sum into `out`
int camera_piece(rb_engine* e, const rb::KParams& p, const rb_camera_ex& cam, uint64_t first_pixel, size_t done, size_t m,
                 uint32_t first_sample, uint32_t samples, rb_radiance* out, rb::LaunchInfo* li) {
    while (e->ev_cam.size() < 2 * (e->cam_pieces + 1)) {
        hipEvent_t x = nullptr;
        if (const hipError_t st = hipEventCreate(&x)) return static_cast<int>(st);
        e->ev_cam.push_back(x);
    }
    hipEvent_t* const ev = &e->ev_cam[2 * e->cam_pieces];
    rb::CamGenArgs g{};
    g.cam = cam;
    g.recs = e->q_rays.ptr;
    g.first_pixel = static_cast<uint32_t>(first_pixel + done);
    g.n = static_cast<uint32_t>(m);
    g.first_sample = first_sample;
    g.samples = samples;
    if (const hipError_t st = hipEventRecord(ev[0], e->stream)) return static_cast<int>(st);
    const int st = rb::launch_camera_rays(g, e->stream);
    if (st) return st;
    if (const hipError_t st1 = hipEventRecord(ev[1], e->stream)) return static_cast<int>(st1);
    e->cam_pieces++;
    return rb::launch_radiance(p, trace_args(e, e->q_rays.ptr, nullptr, out, done, m, first_sample, samples), e->stream, li, true);
}

int trace_camera_locked(rb_engine* e, const rb_camera_ex& cam, uint64_t first_pixel, size_t n, uint32_t first_sample, uint32_t samples,
                        rb_radiance* out) {
    rb::KParams p{};
    int rc = query_params(e, &p);
    e->last_query_ms = 0.0f;
    e->cam_pieces = 0;
    if (rc || n == 0) return rc;
    const size_t piece = std::min(n, camera_piece_pixels(samples));
    rc = camera_scratch(e, piece, samples);
    if (rc) return rc;
    HIP_TRY(e, e->rad_out.reserve(piece));
    const bool pinned = page_locked(out);
    for (size_t done = 0; done < n; done += piece) {
        const size_t m = std::min(piece, n - done);
        rb::LaunchInfo li{};
        HIP_TRY(e, hipEventRecord(e->ev_q[0], e->stream));
        const int st = camera_piece(e, p, cam, first_pixel, done, m, first_sample, samples, e->rad_out.ptr, &li);
        if (st) return rb::fail(e, RB_ERR_DEVICE, "camera kernel launch failed: %s", hipGetErrorString(static_cast<hipError_t>(st)));
        HIP_TRY(e, hipEventRecord(e->ev_q[1], e->stream));
        if (li.kernel_name) e->last_query_kernel_name = li.kernel_name;
        rc = query_copy_out(e, out + done, e->rad_out.ptr, m * sizeof(rb_radiance), pinned);
        if (rc) return rc;
        HIP_TRY(e, hipStreamSynchronize(e->stream));   // the scratch is the next piece's
        float ms = 0.0f;
        HIP_TRY(e, hipEventElapsedTime(&ms, e->ev_q[0], e->ev_q[1]));
        e->last_query_ms += ms;
    }
    return RB_OK;
}

// every piece queued between the query's two events (the pieces share the scratch in stream order); nothing is waited for
int trace_camera_device_locked(rb_engine* e, const rb_camera_ex& cam, uint64_t first_pixel, size_t n, uint32_t first_sample,
                               uint32_t samples, rb_radiance* d_out) {
    const int rc = device_range(e, d_out, n * sizeof(rb_radiance), 16, "d_out");
    if (rc) return rc;
    const size_t piece = std::min(n, camera_piece_pixels(samples));
    e->cam_pieces = 0;
    return device_query_locked(e, [&](const rb::KParams& p, rb::LaunchInfo* li) {
        if (camera_scratch(e, piece, samples)) return static_cast<int>(hipErrorOutOfMemory);
        for (size_t done = 0; done < n; done += piece) {
            const int st = camera_piece(e, p, cam, first_pixel, done, std::min(piece, n - done), first_sample, samples, d_out + done, li);
            if (st) return st;
        }
        return 0;
    });
}

// the refusals every camera entry point shares; before a device is touched (e may be NULL: rb_camera_rays)
int camera_check(rb_engine* e, const char* who, const rb_camera_ex* cam, uint64_t first_pixel, size_t n, uint32_t first_sample, uint32_t samples) {
    const rb_camera_ex& c = *cam;
    if (c.kind != RB_CAM_PERSPECTIVE && c.kind != RB_CAM_ORTHO && c.kind != RB_CAM_EQUIRECT)
        return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: unknown camera kind %u", who, c.kind);
    if ((c.flags & ~static_cast<uint32_t>(RB_CAM_NO_JITTER)) != 0u) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: unknown flag bits 0x%x", who, c.flags);
    if (c._reserved[0] || c._reserved[1] || c._reserved[2]) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: _reserved must be 0", who);
    if (c.width == 0u || c.height == 0u || c.width > (1u << 24) || c.height > (1u << 24))
        return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: width and height are 1 .. 2^24, not %u x %u", who, c.width, c.height);
    const uint64_t pixels = static_cast<uint64_t>(c.width) * c.height;
    if (pixels >= (1ull << 31)) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: an image of %u x %u pixels is too large", who, c.width, c.height);
    if (first_pixel > pixels || n > pixels - first_pixel)
        return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: pixels [%llu, +%zu) leave the image of %llu pixels", who,
                        static_cast<unsigned long long>(first_pixel), n, static_cast<unsigned long long>(pixels));
    if (samples == 0 || samples > 65536u) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s takes 1 .. 65536 samples per pixel, not %u", who, samples);
    if (static_cast<uint64_t>(first_sample) + samples > 0xFFFFFFFFull)
        return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: first_sample + samples = %u + %u does not fit 32 bits", who, first_sample, samples);
    if (static_cast<uint64_t>(n) * samples > 0x7FFFFFFFull - 63ull)
        return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s takes at most 2^31 - 64 (pixel, sample) items per call", who);
    // (pos may be non-finite: its rays are invalid by rb_cast_rays' rule and weigh 0)
    const float* const basis[] = {c.right, c.up, c.forward};
    bool finite = std::isfinite(c.tan_half_fov) && std::isfinite(c.half_width) && std::isfinite(c.half_height) &&
                  std::isfinite(c.lens_radius) && std::isfinite(c.focus_distance);
    for (const float* v : basis) finite = finite && std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]);
    if (!finite) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: a field of the camera other than pos is not finite", who);
    if (c.kind == RB_CAM_PERSPECTIVE && (!(c.tan_half_fov > 0.0f) || c.lens_radius < 0.0f || (c.lens_radius > 0.0f && !(c.focus_distance > 0.0f))))
        return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: a perspective camera needs tan_half_fov > 0, lens_radius >= 0 and, with a lens, focus_distance > 0", who);
    if (c.kind == RB_CAM_ORTHO && (!(c.half_width > 0.0f) || !(c.half_height > 0.0f)))
        return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: an orthographic camera needs half_width > 0 and half_height > 0", who);
    return RB_OK;
}

// ---- the denoiser (rb_abi.h).  Like a query it is queued on the engine's stream behind whatever runs
// there, reads the scene and the committed accumulation, and writes buffers of its own.
rb::GuidePlanes guide_planes(rb_engine* e) { return rb::GuidePlanes{e->dn_nt.ptr, e->dn_pc.ptr, e->dn_al.ptr}; }

int denoise_ready(rb_engine* e) {
    if (rb::is_group(e)) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "the denoiser does not take a multi-device handle: a tap would cross a stripe boundary");
    rb::set_device(e);
    if (e->opt.shard_count > 1) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "the denoiser does not take a sharded engine: a tap would cross a stripe boundary");
    const int rc = require_ready(e);
    if (rc) return rc;
    for (hipEvent_t& x : e->ev_dn)
        if (!x) HIP_TRY(e, hipEventCreate(&x));
    return RB_OK;
}

// the guide planes of the current scene: the pixel-centre rays through the query kernels straight into device memory, one pack
int ensure_guides(rb_engine* e) {
    e->last_guide_ms = 0.0f;
    if (e->dn_guides_valid) return RB_OK;
    int rc = ensure_prepared(e);
    if (rc) return rc;
    rb::KParams p = make_params(e, 0, 0, e->cur, e->cur);
    if (!e->stack_depth_covers) return rb::fail(e, RB_ERR_DEVICE, "internal: a traversal is deeper than its LDS stack column (%u entries)", p.stack_depth);
    const uint32_t w = e->width, h = e->height;
    const size_t n = static_cast<size_t>(w) * h;
    rb::DevBuf<rb_hit> hits;       // the records live until the pack has read them
    rb::DevBuf<rb_surface> surf;
    HIP_TRY(e, hits.resize(n));
    HIP_TRY(e, surf.resize(n));
    HIP_TRY(e, e->dn_nt.resize(n * 4));
    HIP_TRY(e, e->dn_pc.resize(n * 4));
    HIP_TRY(e, e->dn_al.resize(n * 4));
    if (n) {
        HIP_TRY(e, hipEventRecord(e->ev_dn[0], e->stream));
        const uint32_t piece_rows = std::max<uint32_t>(8u, (rb::kQueryPiece / w) & ~7u);   // whole 8-row tiles, as rb_render_hits
        for (uint32_t r0 = 0; r0 < h; r0 += piece_rows) {
            rb::QueryArgs q{};
            q.win_y = r0;
            q.win_w = w;
            q.win_h = std::min(piece_rows, h - r0);
            q.win_global = 1u;
            q.hits = hits.ptr + static_cast<size_t>(r0) * w;
            q.surf = surf.ptr + static_cast<size_t>(r0) * w;
            const int st = rb::launch_query(p, q, e->stream, nullptr);
            if (st) return rb::fail(e, RB_ERR_DEVICE, "query kernel launch failed: %s", hipGetErrorString(static_cast<hipError_t>(st)));
        }
        const int st = rb::launch_guide_pack(p.u, hits.ptr, surf.ptr, w, h, guide_planes(e), e->stream);
        if (st) return rb::fail(e, RB_ERR_DEVICE, "guide pack launch failed: %s", hipGetErrorString(static_cast<hipError_t>(st)));
        HIP_TRY(e, hipEventRecord(e->ev_dn[1], e->stream));
        HIP_TRY(e, hipStreamSynchronize(e->stream));
        HIP_TRY(e, hipEventElapsedTime(&e->last_guide_ms, e->ev_dn[0], e->ev_dn[1]));
    }
    e->dn_guides_valid = true;
    return RB_OK;
}

int denoise_params_check(const rb_engine* e, const rb_denoise_params* prm) {
    const char* why = nullptr;
    if (!rb::denoise_params_valid(*prm, &why)) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "rb_denoise_params: %s", why);
    return RB_OK;
}

// device == true: the outputs are the caller's device buffers and nothing is waited for
int denoise_locked(rb_engine* e, const rb_denoise_params* prm, uint8_t* rgba_out, float* linear_out, bool device) {
    int rc = denoise_ready(e);
    if (!rc) rc = denoise_params_check(e, prm);
    if (rc) return rc;
    if (!rgba_out && !linear_out) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "rgba_out and linear_out are both NULL");
    const size_t n = static_cast<size_t>(e->width) * e->height;
    if (device) {
        if (rgba_out) rc = device_range(e, rgba_out, n * 4, 4, "d_rgba_out");
        if (!rc && linear_out) rc = device_range(e, linear_out, n * 16, 16, "d_linear_out");
        if (rc) return rc;
    }
    rc = ensure_guides(e);
    if (rc) return rc;
    e->denoise_ms_pending = false;
    e->last_denoise_ms = 0.0f;
    if (n == 0) return RB_OK;
    rb::DenoiseArgs a{};
    a.w = e->width;
    a.h = e->height;
    a.accum = e->slot[e->cur].accum.ptr;
    a.g = guide_planes(e);
    for (int k = 0; k < 2; ++k) {
        HIP_TRY(e, e->dn_r[k].resize(n * 4));
        a.r[k] = e->dn_r[k].ptr;
    }
    if (device) {
        a.rgba_out = reinterpret_cast<uint32_t*>(rgba_out);
        a.linear_out = linear_out;
    } else {
        if (rgba_out) {
            HIP_TRY(e, e->dn_rgba.resize(n));
            a.rgba_out = e->dn_rgba.ptr;
        }
        if (linear_out) {
            HIP_TRY(e, e->dn_linear.resize(n * 4));
            a.linear_out = e->dn_linear.ptr;
        }
    }
    HIP_TRY(e, hipEventRecord(e->ev_dn[2], e->stream));
    const int st = rb::launch_denoise(*prm, a, e->stream);
    if (st) return rb::fail(e, RB_ERR_DEVICE, "denoise kernel launch failed: %s", hipGetErrorString(static_cast<hipError_t>(st)));
    HIP_TRY(e, hipEventRecord(e->ev_dn[3], e->stream));
    if (device) {
        e->denoise_ms_pending = true;
        return RB_OK;
    }
    if (rgba_out) rc = query_copy_out(e, rgba_out, e->dn_rgba.ptr, n * 4, page_locked(rgba_out));
    if (!rc && linear_out) rc = query_copy_out(e, linear_out, e->dn_linear.ptr, n * 16, page_locked(linear_out));
    if (rc) return rc;
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    HIP_TRY(e, hipEventElapsedTime(&e->last_denoise_ms, e->ev_dn[2], e->ev_dn[3]));
    return RB_OK;
}

int denoise_guides_locked(rb_engine* e, rb_guide* guides_out) {
    int rc = denoise_ready(e);
    if (!rc) rc = ensure_guides(e);
    if (rc) return rc;
    const size_t n = static_cast<size_t>(e->width) * e->height;
    if (n == 0) return RB_OK;
    rb::DevBuf<rb_guide> joined;
    HIP_TRY(e, joined.resize(n));
    const int st = rb::launch_guide_join(guide_planes(e), n, joined.ptr, e->stream);
    if (st) return rb::fail(e, RB_ERR_DEVICE, "guide join launch failed: %s", hipGetErrorString(static_cast<hipError_t>(st)));
    rc = query_copy_out(e, guides_out, joined.ptr, n * sizeof(rb_guide), page_locked(guides_out));
    if (rc) return rc;
    HIP_TRY(e, hipStreamSynchronize(e->stream));   // `joined` is freed on return
    return RB_OK;
}

// the engine that answers a query (a multi-device handle: devices[0], which holds the whole scene), made current
rb_engine* answering(rb_engine* e) {
    rb_engine* const t = rb::is_group(e) ? e->parts[0].get() : e;
    rb::set_device(t);
    return t;
}

int answered(rb_engine* e, rb_engine* t, int rc) {
    if (rc && t != e) copy_error(e, t);
    return rc;
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
    // every launch, copy and event record of this engine was queued on its one stream: when that has
    // drained nothing on the device refers to the buffers, events or communicator any more
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    if (e->copy_stream) {
        (void)hipStreamSynchronize(e->copy_stream);
        (void)hipStreamDestroy(e->copy_stream);
    }
    rb::gather_destroy(e->net);
    if (e->ev_begin) (void)hipEventDestroy(e->ev_begin);
    if (e->ev_end) (void)hipEventDestroy(e->ev_end);
    for (rb::FrameSlot& s : e->slot)
        if (s.done) (void)hipEventDestroy(s.done);
    for (hipEvent_t x : e->ev_pool) (void)hipEventDestroy(x);
    for (hipEvent_t x : e->ev_cam) (void)hipEventDestroy(x);
    for (hipEvent_t x : e->ev_q)
        if (x) (void)hipEventDestroy(x);
    for (hipEvent_t x : e->ev_dn)
        if (x) (void)hipEventDestroy(x);
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
    if (!e->have_uniforms) return rb::fail(e, RB_ERR_UNIFORMS_NOT_INITIALIZED, "Uniforms must be initialized");  // gpu_wrapper.rs:313,321
    if (width) *width = e->width;
    if (height) *height = e->height;
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
        uint32_t chunk = 0;
        if (!rc) rc = reserve_colors(p, n_passes, &chunk);
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
        const uint32_t w = p0->width, h = p0->height, sr = p0->opt.stripe_rows ? p0->opt.stripe_rows : rb::kDefaultStripeRows;
        const uint32_t n = static_cast<uint32_t>(e->parts.size());
        std::vector<float> tmp(static_cast<size_t>(w) * p0->padded_rows * 4);
        for (uint32_t r = 0; r < n; ++r) {
            rb_engine* p = e->parts[r].get();
            PART_TRY(e, p, require_ready(p));
            HIP_TRY(e, hipStreamSynchronize(p->stream));
            HIP_TRY(e, hipMemcpy(tmp.data(), p->slot[p->cur].accum.ptr, tmp.size() * sizeof(float), hipMemcpyDeviceToHost));
            for (uint32_t lr = 0; lr < p->padded_rows; ++lr) {
                const uint32_t y = ((lr / sr) * n + r) * sr + lr % sr;
                if (y < h) std::memcpy(accum_out + static_cast<size_t>(y) * w * 4, tmp.data() + static_cast<size_t>(lr) * w * 4, static_cast<size_t>(w) * 16);
            }
        }
        return RB_OK;
    }
    rb::set_device(e);
    int rc = require_ready(e);
    if (rc) return rc;
    const uint32_t rows = (e->opt.shard_count > 1) ? e->padded_rows : e->height;
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    HIP_TRY(e, hipMemcpy(accum_out, e->slot[e->cur].accum.ptr, static_cast<size_t>(e->width) * rows * 16, hipMemcpyDeviceToHost));
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
        if (bytes) *bytes = static_cast<size_t>(e->width) * e->height * 4;
        return RB_OK;
    }
    if (d_ptr) *d_ptr = e->slot[e->cur].rgba.ptr;
    if (bytes) *bytes = static_cast<size_t>(e->width) * e->padded_rows * 4;
    return RB_OK;
}

int rb_local_rows(const rb_engine* e, uint32_t* rows, uint32_t* padded_rows) {
    if (!e) return RB_ERR_NULL_ARGUMENT;
    if (rb::is_group(e)) {  // the handle delivers whole frames
        if (rows) *rows = e->height;
        if (padded_rows) *padded_rows = e->height;
        return RB_OK;
    }
    const uint32_t sc = e->opt.shard_count > 1 ? e->opt.shard_count : 1;
    const uint32_t sr = e->opt.stripe_rows ? e->opt.stripe_rows : rb::kDefaultStripeRows;
    uint32_t owned = e->height;
    if (sc > 1) {
        owned = 0;
        const uint32_t stripes = (e->height + sr - 1) / sr;
        for (uint32_t s = e->opt.shard_rank; s < stripes; s += sc) owned += std::min(sr, e->height - s * sr);
    }
    if (rows) *rows = owned;
    if (padded_rows) *padded_rows = e->padded_rows;
    return RB_OK;
}

int rb_global_row(const rb_engine* e, uint32_t local_row, uint32_t* global_row) {
    if (!e || !global_row) return RB_ERR_NULL_ARGUMENT;
    if (rb::is_group(e)) { *global_row = local_row; return RB_OK; }
    const uint32_t sc = e->opt.shard_count > 1 ? e->opt.shard_count : 1;
    const uint32_t sr = e->opt.stripe_rows ? e->opt.stripe_rows : rb::kDefaultStripeRows;
    if (sc == 1) { *global_row = local_row; return RB_OK; }
    *global_row = ((local_row / sr) * sc + e->opt.shard_rank) * sr + local_row % sr;
    return RB_OK;
}

int rb_shard_layout(uint32_t height, uint32_t shard_rank, uint32_t shard_count, uint32_t stripe_rows,
                    uint32_t* owned_rows, uint32_t* padded_rows) {
    const uint32_t sc = shard_count > 1 ? shard_count : 1;
    const uint32_t sr = stripe_rows ? stripe_rows : rb::kDefaultStripeRows;
    if (shard_rank >= sc) return RB_ERR_INVALID_OPTIONS;
    uint32_t owned = height, padded = height;
    if (sc > 1) {
        const uint32_t stripes = (height + sr - 1) / sr;
        padded = ((stripes + sc - 1) / sc) * sr;
        owned = 0;
        for (uint32_t s = shard_rank; s < stripes; s += sc) owned += std::min(sr, height - s * sr);
    }
    if (owned_rows) *owned_rows = owned;
    if (padded_rows) *padded_rows = padded;
    return RB_OK;
}

uint32_t rb_shard_global_row(uint32_t shard_rank, uint32_t shard_count, uint32_t stripe_rows, uint32_t local_row) {
    const uint32_t sc = shard_count > 1 ? shard_count : 1;
    const uint32_t sr = stripe_rows ? stripe_rows : rb::kDefaultStripeRows;
    if (sc == 1) return local_row;
    return ((local_row / sr) * sc + shard_rank) * sr + local_row % sr;
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

int rb_cast_rays(rb_engine* e, const rb_ray* rays, size_t n, rb_hit* hits_out, rb_surface* surf_out) {
    if (!e) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    if (n > 0x7FFFFFFFull - 63ull) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "rb_cast_rays takes at most 2^31 - 64 rays per call");
    if (n > 0 && (!rays || !hits_out)) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "rays / hits_out is NULL");
    if (rb::is_group(e)) {   // every part holds the whole scene
        rb_engine* p0 = e->parts[0].get();
        PART_TRY(e, p0, cast_rays_locked(p0, rays, n, hits_out, surf_out));
        return RB_OK;
    }
    rb::set_device(e);
    return cast_rays_locked(e, rays, n, hits_out, surf_out);
}

int rb_render_hits(rb_engine* e, rb_hit* hits_out, rb_surface* surf_out) {
    if (!e) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    if (!hits_out) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "hits_out is NULL");
    if (rb::is_group(e)) {   // the whole frame on devices[0]: one ray per pixel is not worth a gather
        rb_engine* p0 = e->parts[0].get();
        PART_TRY(e, p0, require_ready(p0));
        PART_TRY(e, p0, pixel_hits_locked(p0, 0, 0, p0->width, p0->height, true, hits_out, surf_out));
        return RB_OK;
    }
    rb::set_device(e);
    int rc = require_ready(e);
    if (rc) return rc;
    const bool sharded = e->opt.shard_count > 1;
    return pixel_hits_locked(e, 0, 0, e->width, sharded ? e->padded_rows : e->height, !sharded, hits_out, surf_out);
}

int rb_pick(rb_engine* e, uint32_t px, uint32_t py, rb_hit* hit_out, rb_surface* surf_out) {
    if (!e) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    if (!hit_out) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "hit_out is NULL");
    rb_engine* t = rb::is_group(e) ? e->parts[0].get() : e;
    rb::set_device(t);
    int rc = require_ready(t);
    if (!rc && (px >= t->width || py >= t->height)) rc = rb::fail(t, RB_ERR_INVALID_OPTIONS, "pixel (%u, %u) is outside the %u x %u image", px, py, t->width, t->height);
    if (!rc) rc = pixel_hits_locked(t, px, py, 1, 1, true, hit_out, surf_out);
    if (rc && t != e) copy_error(e, t);
    return rc;
}

int rb_occluded(rb_engine* e, const rb_ray* rays, const float* tmax, size_t n, uint32_t mask, uint8_t* out) {
    if (!e) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    if (n > 0x7FFFFFFFull - 63ull) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "rb_occluded takes at most 2^31 - 64 rays per call");
    if (mask > RB_MASK_ALL) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "mask has bits above RB_MASK_ALL");
    if (n > 0 && (!rays || !out)) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "rays / out is NULL");
    rb_engine* const t = answering(e);
    return answered(e, t, occluded_locked(t, rays, tmax, n, mask, out));
}

int rb_occluded_device(rb_engine* e, const rb_ray* d_rays, const float* d_tmax, size_t n, uint32_t mask, uint8_t* d_out) {
    if (!e) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    if (n > 0x7FFFFFFFull - 63ull) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "rb_occluded_device takes at most 2^31 - 64 rays per call");
    if (mask > RB_MASK_ALL) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "mask has bits above RB_MASK_ALL");
    if (n > 0 && (!d_rays || !d_out)) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "d_rays / d_out is NULL");
    rb_engine* const t = answering(e);
    if (n == 0) return answered(e, t, require_ready(t));
    return answered(e, t, occluded_device_locked(t, d_rays, d_tmax, n, mask, d_out));
}

int rb_cast_rays_device(rb_engine* e, const rb_ray* d_rays, size_t n, rb_hit* d_hits, rb_surface* d_surf) {
    if (!e) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    if (n > 0x7FFFFFFFull - 63ull) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "rb_cast_rays_device takes at most 2^31 - 64 rays per call");
    if (n > 0 && (!d_rays || !d_hits)) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "d_rays / d_hits is NULL");
    rb_engine* const t = answering(e);
    if (n == 0) return answered(e, t, require_ready(t));
    return answered(e, t, cast_rays_device_locked(t, d_rays, n, d_hits, d_surf));
}

// the refusals the two forms of rb_trace_rays share; before any launch
static int trace_rays_check(rb_engine* e, const char* who, const void* rays, size_t n, uint32_t first_sample, uint32_t samples, const void* out) {
    if (samples == 0 || samples > 65536u) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s takes 1 .. 65536 samples per ray, not %u", who, samples);
    if (static_cast<uint64_t>(first_sample) + samples > 0xFFFFFFFFull)
        return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: first_sample + samples = %u + %u does not fit 32 bits", who, first_sample, samples);
    if (n > 0x7FFFFFFFull - 63ull) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s takes at most 2^31 - 64 rays per call", who);
    if (n > 0 && (!rays || !out)) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: rays / out is NULL", who);
    return RB_OK;
}

int rb_trace_rays(rb_engine* e, const rb_ray* rays, const uint32_t* seeds, size_t n, uint32_t first_sample, uint32_t samples,
                  rb_radiance* out) {
    if (!e) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    if (const int rc = trace_rays_check(e, "rb_trace_rays", rays, n, first_sample, samples, out)) return rc;
    rb_engine* const t = answering(e);
    return answered(e, t, trace_rays_locked(t, rays, seeds, n, first_sample, samples, out));
}

int rb_trace_rays_device(rb_engine* e, const rb_ray* d_rays, const uint32_t* d_seeds, size_t n, uint32_t first_sample,
                         uint32_t samples, rb_radiance* d_out) {
    if (!e) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    if (const int rc = trace_rays_check(e, "rb_trace_rays_device", d_rays, n, first_sample, samples, d_out)) return rc;
    rb_engine* const t = answering(e);
    if (n == 0) return answered(e, t, require_ready(t));
    return answered(e, t, trace_rays_device_locked(t, d_rays, d_seeds, n, first_sample, samples, d_out));
}

int rb_camera_rays(int32_t device, const rb_camera_ex* cam, uint64_t first_pixel, size_t n_pixels, uint32_t first_sample,
                   uint32_t samples, rb_ray* rays_out, uint32_t* seeds_out) {
    if (n_pixels > 0 && (!cam || !rays_out || !seeds_out)) return rb::fail(nullptr, RB_ERR_NULL_ARGUMENT, "cam / rays_out / seeds_out is NULL");
    if (cam)
        if (const int rc = camera_check(nullptr, "rb_camera_rays", cam, first_pixel, n_pixels, first_sample, samples)) return rc;
    if (n_pixels == 0) return RB_OK;
    if (device >= 0 && hipSetDevice(device) != hipSuccess) return rb::fail(nullptr, RB_ERR_DEVICE, "hipSetDevice(%d) failed", device);
    const size_t items = n_pixels * samples, piece = std::min<size_t>(items, size_t(1) << 22);   // 128 + 16 MiB of scratch
    rb::DevBuf<rb_ray> d_rays;
    rb::DevBuf<uint32_t> d_seeds;
    hipStream_t stream = nullptr;
    hipError_t st = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
    if (st == hipSuccess) st = d_rays.resize(piece);
    if (st == hipSuccess) st = d_seeds.resize(piece);
    for (size_t done = 0; done < items && st == hipSuccess; done += piece) {
        const size_t m = std::min(piece, items - done);
        rb::CamGenArgs g{};
        g.cam = *cam;
        g.recs = d_rays.ptr;
        g.seeds = d_seeds.ptr;
        g.first_pixel = static_cast<uint32_t>(first_pixel);
        g.n = static_cast<uint32_t>(m);
        g.item_base = static_cast<uint32_t>(done);
        g.first_sample = first_sample;
        g.samples = samples;
        g.linear = 1u;
        st = static_cast<hipError_t>(rb::launch_camera_rays(g, stream));
        if (st == hipSuccess) st = hipMemcpyAsync(rays_out + done, d_rays.ptr, m * sizeof(rb_ray), hipMemcpyDeviceToHost, stream);
        if (st == hipSuccess) st = hipMemcpyAsync(seeds_out + done, d_seeds.ptr, m * sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
        if (st == hipSuccess) st = hipStreamSynchronize(stream);   // the scratch is the next piece's
    }
    if (stream) (void)hipStreamSynchronize(stream);   // (the buffers are freed on return, after this)
    if (stream) (void)hipStreamDestroy(stream);
    if (st != hipSuccess) return rb::fail(nullptr, RB_ERR_DEVICE, "rb_camera_rays failed: %s", hipGetErrorString(st));
    return RB_OK;
}

int rb_trace_camera(rb_engine* e, const rb_camera_ex* cam, uint64_t first_pixel, size_t n_pixels, uint32_t first_sample,
                    uint32_t samples, rb_radiance* out) {
    if (!e) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    if (n_pixels > 0 && (!cam || !out)) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "rb_trace_camera: cam / out is NULL");
    if (cam)
        if (const int rc = camera_check(e, "rb_trace_camera", cam, first_pixel, n_pixels, first_sample, samples)) return rc;
    rb_engine* const t = answering(e);
    if (n_pixels == 0) return answered(e, t, require_ready(t));
    return answered(e, t, trace_camera_locked(t, *cam, first_pixel, n_pixels, first_sample, samples, out));
}

int rb_trace_camera_device(rb_engine* e, const rb_camera_ex* cam, uint64_t first_pixel, size_t n_pixels, uint32_t first_sample,
                           uint32_t samples, rb_radiance* d_out) {
    if (!e) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    if (n_pixels > 0 && (!cam || !d_out)) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "rb_trace_camera_device: cam / d_out is NULL");
    if (cam)
        if (const int rc = camera_check(e, "rb_trace_camera_device", cam, first_pixel, n_pixels, first_sample, samples)) return rc;
    rb_engine* const t = answering(e);
    if (n_pixels == 0) return answered(e, t, require_ready(t));
    return answered(e, t, trace_camera_device_locked(t, *cam, first_pixel, n_pixels, first_sample, samples, d_out));
}

int rb_denoise_default_params(rb_denoise_params* p) {
    if (!p) return RB_ERR_NULL_ARGUMENT;
    *p = rb_denoise_params{};
    p->iterations = 3;   // chosen on the quality test: DESIGN.md section 13.4
    p->normal_power_log2 = 3;
    p->sigma_depth = 0.02f;
    p->sigma_color = 0.0f;   // the colour term is off: at a few samples per pixel it takes fireflies for edges
    p->albedo_floor = 0.01f;
    return RB_OK;
}

int rb_denoise(rb_engine* e, const rb_denoise_params* params, uint8_t* rgba_out, float* linear_out) {
    if (!e || !params) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    return denoise_locked(e, params, rgba_out, linear_out, false);
}

int rb_denoise_device(rb_engine* e, const rb_denoise_params* params, uint8_t* d_rgba_out, float* d_linear_out) {
    if (!e || !params) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    return denoise_locked(e, params, d_rgba_out, d_linear_out, true);
}

int rb_denoise_guides(rb_engine* e, rb_guide* guides_out) {
    if (!e) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    if (!guides_out) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "guides_out is NULL");
    return denoise_guides_locked(e, guides_out);
}

int rb_last_denoise_ms(rb_engine* e, float* ms, float* guide_build_ms) {
    if (!e || !ms) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    if (e->denoise_ms_pending) {   // rb_denoise_device returned without waiting: its events are read here
        rb::set_device(e);
        HIP_TRY(e, hipEventSynchronize(e->ev_dn[3]));
        HIP_TRY(e, hipEventElapsedTime(&e->last_denoise_ms, e->ev_dn[2], e->ev_dn[3]));
        e->denoise_ms_pending = false;
    }
    *ms = e->last_denoise_ms;
    if (guide_build_ms) *guide_build_ms = e->last_guide_ms;
    return RB_OK;
}

int rb_denoise_buffers(int32_t device, const rb_denoise_params* params, uint32_t w, uint32_t h, const float* color4,
                       const rb_guide* guides, float* out4, uint8_t* rgba_out) {
    if (!params || !color4 || !guides) return rb::fail(nullptr, RB_ERR_NULL_ARGUMENT, "params / color4 / guides is NULL");
    if (!out4 && !rgba_out) return rb::fail(nullptr, RB_ERR_NULL_ARGUMENT, "out4 and rgba_out are both NULL");
    if (const int rc = denoise_params_check(nullptr, params)) return rc;
    const size_t n = static_cast<size_t>(w) * h;
    if (n >= (1ull << 31)) return rb::fail(nullptr, RB_ERR_INVALID_OPTIONS, "a frame of %u x %u pixels is too large", w, h);
    if (n == 0) return RB_OK;
    if (device >= 0 && hipSetDevice(device) != hipSuccess) return rb::fail(nullptr, RB_ERR_DEVICE, "hipSetDevice(%d) failed", device);
    rb::DevBuf<float> d_color, d_nt, d_pc, d_al, d_r0, d_r1, d_linear;
    rb::DevBuf<rb_guide> d_guides;
    rb::DevBuf<uint32_t> d_rgba;
    hipStream_t stream = nullptr;
    hipError_t st = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
    for (rb::DevBuf<float>* b : {&d_color, &d_nt, &d_pc, &d_al, &d_r0, &d_r1})
        if (st == hipSuccess) st = b->resize(n * 4);
    if (st == hipSuccess) st = d_guides.resize(n);
    if (st == hipSuccess && out4) st = d_linear.resize(n * 4);
    if (st == hipSuccess && rgba_out) st = d_rgba.resize(n);
    if (st == hipSuccess) st = hipMemcpyAsync(d_color.ptr, color4, n * 16, hipMemcpyHostToDevice, stream);
    if (st == hipSuccess) st = hipMemcpyAsync(d_guides.ptr, guides, n * sizeof(rb_guide), hipMemcpyHostToDevice, stream);
    rb::DenoiseArgs a{};
    a.w = w;
    a.h = h;
    a.color4 = d_color.ptr;
    a.g = rb::GuidePlanes{d_nt.ptr, d_pc.ptr, d_al.ptr};
    a.r[0] = d_r0.ptr;
    a.r[1] = d_r1.ptr;
    a.linear_out = d_linear.ptr;
    a.rgba_out = d_rgba.ptr;
    if (st == hipSuccess) st = static_cast<hipError_t>(rb::launch_guide_split(d_guides.ptr, n, a.g, stream));
    if (st == hipSuccess) st = static_cast<hipError_t>(rb::launch_denoise(*params, a, stream));
    if (st == hipSuccess && out4) st = hipMemcpyAsync(out4, d_linear.ptr, n * 16, hipMemcpyDeviceToHost, stream);
    if (st == hipSuccess && rgba_out) st = hipMemcpyAsync(rgba_out, d_rgba.ptr, n * 4, hipMemcpyDeviceToHost, stream);
    if (st == hipSuccess) st = hipStreamSynchronize(stream);
    if (stream) (void)hipStreamSynchronize(stream);   // (the buffers are freed on return, after this)
    if (stream) (void)hipStreamDestroy(stream);
    if (st != hipSuccess) return rb::fail(nullptr, RB_ERR_DEVICE, "rb_denoise_buffers failed: %s", hipGetErrorString(st));
    return RB_OK;
}

const char* rb_last_query_kernel_name(const rb_engine* e) {
    if (!e) return "";
    return rb::is_group(e) ? e->parts[0]->last_query_kernel_name : e->last_query_kernel_name;
}

int rb_last_query_ms(rb_engine* e, float* ms) {
    if (!e || !ms) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    rb_engine* const t = rb::is_group(e) ? e->parts[0].get() : e;
    if (t->query_ms_pending) {   // a device form returned without waiting: its events are read here
        rb::set_device(t);
        HIP_TRY(e, hipEventSynchronize(t->ev_q[1]));
        HIP_TRY(e, hipEventElapsedTime(&t->last_query_ms, t->ev_q[0], t->ev_q[1]));
        t->query_ms_pending = false;
    }
    *ms = t->last_query_ms;
    return RB_OK;
}

int rb_last_camera_rays_ms(rb_engine* e, float* ms) {
    if (!e || !ms) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    rb_engine* const t = rb::is_group(e) ? e->parts[0].get() : e;
    *ms = 0.0f;
    if (t->cam_pieces == 0) return RB_OK;
    rb::set_device(t);
    HIP_TRY(e, hipEventSynchronize(t->ev_cam[2 * t->cam_pieces - 1]));
    for (size_t i = 0; i < t->cam_pieces; i++) {
        float piece_ms = 0.0f;
        HIP_TRY(e, hipEventElapsedTime(&piece_ms, t->ev_cam[2 * i], t->ev_cam[2 * i + 1]));
        *ms += piece_ms;
    }
    return RB_OK;
}

const char* rb_last_kernel_name(const rb_engine* e) {
    if (!e) return "";
    return rb::is_group(e) ? e->parts[0]->last_kernel_name : e->last_kernel_name;
}

int rb_device_name(int device, char* buf, size_t buf_len) {
    if (!buf || buf_len == 0) return RB_ERR_NULL_ARGUMENT;
    hipDeviceProp_t prop;
    if (device < 0 && hipGetDevice(&device) != hipSuccess) return RB_ERR_DEVICE;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return RB_ERR_DEVICE;
    snprintf(buf, buf_len, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    return RB_OK;
}

// Test hook: exhaustive device check of the fast reciprocal (all 2^23 significands, both signs)
// at one biased exponent.  out16[0] = number of mismatches, out16[1..15] = offending bit patterns.
int rb_debug_rcp_exhaustive(uint32_t biased_exponent, uint32_t* out16) {
    if (!out16) return RB_ERR_NULL_ARGUMENT;
    uint32_t* d = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&d), 64) != hipSuccess) return RB_ERR_DEVICE;
    (void)hipMemset(d, 0, 64);
    int rc = rb::launch_rcp_exhaustive(biased_exponent, d, nullptr);
    hipError_t st = hipDeviceSynchronize();
    (void)hipMemcpy(out16, d, 64, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    return (rc || st != hipSuccess) ? RB_ERR_DEVICE : RB_OK;
}

// Test hook: device check of the fast exact division over denominators [b_begin, b_begin+b_count)
// x numerators [a_begin, a_begin+a_count) (significands; biased exponents ea / eb).
// out16[0] = mismatch count, then up to 7 (a, b) bit-pattern pairs.
int rb_debug_div_exhaustive(uint32_t b_begin, uint32_t b_count, uint32_t ea, uint32_t eb, uint32_t a_begin,
                            uint32_t a_count, unsigned long long* out16) {
    if (!out16) return RB_ERR_NULL_ARGUMENT;
    unsigned long long* d = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&d), 128) != hipSuccess) return RB_ERR_DEVICE;
    (void)hipMemset(d, 0, 128);
    int rc = rb::launch_div_exhaustive(b_begin, b_count, ea, eb, a_begin, a_count, d, nullptr);
    hipError_t st = hipDeviceSynchronize();
    (void)hipMemcpy(out16, d, 128, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    return (rc || st != hipSuccess) ? RB_ERR_DEVICE : RB_OK;
}

int rb_measure_l1_gather(int32_t device, uint64_t table_bytes, double* accesses_per_s) {
    if (!accesses_per_s) return RB_ERR_NULL_ARGUMENT;
    if (device >= 0 && hipSetDevice(device) != hipSuccess) return RB_ERR_DEVICE;
    *accesses_per_s = rb::measure_l1_gather(table_bytes ? static_cast<size_t>(table_bytes) : (2u << 20), 512u);
    return *accesses_per_s > 0.0 ? RB_OK : RB_ERR_DEVICE;
}

int rb_debug_walk_profile(uint64_t out64[64], int reset) {
    if (!out64) return RB_ERR_NULL_ARGUMENT;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "counter width");
    if (hipDeviceSynchronize() != hipSuccess) return RB_ERR_DEVICE;
    return rb::debug_walk_profile(reinterpret_cast<unsigned long long*>(out64), reset) == 0 ? RB_OK : RB_ERR_DEVICE;
}

// Debug hook for tests/test_gpu_parity.py: device /, sqrt, normalize, u32->f32, min/max, dot.
int rb_debug_math(const float* a, const float* b, float* out8n, uint32_t n) {
    if (!a || !b || !out8n) return RB_ERR_NULL_ARGUMENT;
    float *da = nullptr, *db = nullptr, *dout = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&da), n * 4) != hipSuccess) return RB_ERR_DEVICE;
    if (hipMalloc(reinterpret_cast<void**>(&db), n * 4) != hipSuccess) return RB_ERR_DEVICE;
    if (hipMalloc(reinterpret_cast<void**>(&dout), static_cast<size_t>(n) * 32) != hipSuccess) return RB_ERR_DEVICE;
    (void)hipMemcpy(da, a, n * 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(db, b, n * 4, hipMemcpyHostToDevice);
    int rc = rb::launch_debug_math(da, db, dout, n, nullptr);
    hipError_t st = hipDeviceSynchronize();
    (void)hipMemcpy(out8n, dout, static_cast<size_t>(n) * 32, hipMemcpyDeviceToHost);
    (void)hipFree(da); (void)hipFree(db); (void)hipFree(dout);
    return (rc || st != hipSuccess) ? RB_ERR_DEVICE : RB_OK;
}

}  // extern "C"
