// rb_update_plan.hpp -- what an rb_update decides before a buffer is touched ("The update plan"): the
// nine fields as a table, what the decision knows of the engine (SceneFacts), the plan of one update (plan_update: refusal,
// or per field what is done and the scene that results), the only functions that change the facts (commit_*), the count
// patch-up and the stripe arithmetic of a sharded frame.  Host code only, no HIP: rb_runtime.cpp acts on the plan, and a
// stand-alone program holds it to tests/_update_model.py on the CPU (tests/test_update_plan.py).
//
// The rules are the reference's: RenderConfig::validate_init / validate (render_config.rs:163-268), the Change<T> state
// machine of GpuWrapper::update (gpu_wrapper.rs:116-300) and update_uniforms' count patch-up (:469-495).  On top of them come
// the host-side checks that stand in for WGSL's robust buffer access: anything that would make a HIP kernel read out of
// bounds or loop forever is refused.  They run on the scene the update WOULD leave -- the incoming fields merged with the
// facts -- so a refused rb_update leaves the previous scene live and renderable.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "rb_internal.hpp"

namespace rb {

// ---- the stripes of a sharded frame: rank r of n renders stripes r, r + n, ... of stripe_rows rows each
struct ShardLayout {
    uint32_t rank = 0, count = 1, stripe = kDefaultStripeRows;
    uint32_t whole_rows = 0;    // rows of the stripes this rank renders, whole stripes (the kernels bound rows by global y < height)
    uint32_t owned = 0;         // ... of them inside the image
    uint32_t padded = 0;        // rows of every rank's buffer: equal on all ranks, whole stripes
    uint32_t global_row(uint32_t local) const { return count == 1 ? local : ((local / stripe) * count + rank) * stripe + local % stripe; }
};
inline ShardLayout shard_layout(uint32_t height, uint32_t shard_rank, uint32_t shard_count, uint32_t stripe_rows) {
    ShardLayout l;
    l.rank = shard_rank, l.count = shard_count > 1 ? shard_count : 1, l.stripe = stripe_rows ? stripe_rows : kDefaultStripeRows;
    l.whole_rows = l.owned = l.padded = height;
    if (l.count > 1) {
        const uint32_t stripes = (height + l.stripe - 1) / l.stripe;
        const uint32_t mine = l.rank < stripes ? (stripes - l.rank + l.count - 1) / l.count : 0;
        l.padded = ((stripes + l.count - 1) / l.count) * l.stripe;
        l.whole_rows = l.owned = mine * l.stripe;
        if (mine && (stripes - 1) % l.count == l.rank) l.owned -= stripes * l.stripe - height;   // the image's last stripe may be cut
    }
    return l;
}

// ---- what the decision needs to know of the engine.  rb_engine embeds one (rb_engine::sc): there is no second copy.
struct SceneFacts {
    bool initialized = false;        // GpuWrapper::initialized (gpu_wrapper.rs:69,117)
    bool have_uniforms = false;      // last update carried Create/Update uniforms (:303-329)
    // element counts = what arrayLength() / the patched uniforms see
    uint32_t n_spheres = 0, n_lights = 0, n_meshes = 0, n_nodes = 0, n_indices = 0, n_tris = 0, n_uvs = 0, n_tex = 0;
    // Change of the last update for the three patched counts (gpu_wrapper.rs:475-495)
    uint32_t last_change_spheres = RB_KEEP, last_change_nodes = RB_KEEP, last_change_tris = RB_KEEP;
    // length of the spheres vector the last update carried: a Create after the first update is not acted on, but :476 still
    // takes spheres_count from the vector it was handed (the BVH fields' Create is acted on: their vector is the buffer)
    uint32_t last_spheres_sent = 0;
    uint32_t bvh_stack = 0;          // traversal-stack entries the current tree needs
    uint32_t max_mesh_index = 0;     // over the uploaded triangles
    std::vector<rb_bvh_node> host_nodes;   // kept for validation when nodes/indices change separately
    rb_uniforms uniforms{};          // as handed over (before count patch-up)
    uint32_t width = 0, height = 0, local_rows = 0, padded_rows = 0;
    // of the options, set when the engine is made
    bool own_tree = false;           // RB_FLAG_BUILD_TREE*: the tree follows the triangles field
    uint32_t shard_rank = 0, shard_count = 0, stripe_rows = 0;
    ShardLayout layout(uint32_t h) const { return shard_layout(h, shard_rank, shard_count, stripe_rows); }
    // What the plain walk's flat kernels rest on ("Scenes that carry no u, v"): each is false until the
    // field it reads has been taken, and recomputed (commit_trace_facts) whenever that field is taken or deleted.
    bool untex_meshes = false, untex_spheres = false;   // every material of the field has texture_index < 0
    bool untex_lights = false;       // the same of the lights, the zero-filled phantom of an empty vector (index 0) included
    bool no_uv = false;              // untex_meshes && untex_spheres: no segment reads the winning triangle's u, v
};

// ---- the facts of the flat kernels, from a field's data as the caller hands it over
// every material's texture index is negative.  An index >= n_tex counts as a texture: sample_texture answers it in its texel way.
template <typename T>
inline bool untextured(const T* v, size_t n) {
    if (n > 0 && !v) return false;
    for (size_t i = 0; i < n; ++i)
        if (v[i].material.texture_index >= 0) return false;
    return true;
}

// ---- the field table
enum Field : uint32_t { kUniforms, kSpheres, kUvs, kMeshes, kLights, kNodes, kIndices, kTriangles, kTextures, kFieldCount };
struct Refusal {
    int code;   // RB_OK: none
    const char* text;
};
struct FieldDesc {
    const char* name;
    rb_field rb_config::*member;
    uint32_t SceneFacts::*len;   // its length among the facts (uniforms: none)
    bool bvh;                    // a Create after the first update acts (gpu_wrapper.rs:242-280); elsewhere it is ignored
    Refusal not_create;          // validate_init, where the first config does not create it
    Refusal del;                 // validate, where Delete is refused
};
constexpr Refusal kNoRefusal{RB_OK, ""};
constexpr FieldDesc kFields[kFieldCount] = {
    {"uniforms", &rb_config::uniforms, nullptr, false, {RB_ERR_INVALID_UNIFORMS, "Invalid Uniforms"}, {RB_ERR_CANNOT_DELETE_NONEXISTENT, "Cannot delete none existent"}},
    {"spheres", &rb_config::spheres, &SceneFacts::n_spheres, false, {RB_ERR_INVALID_SPHERES, "Invalid Spheres"}, kNoRefusal},
    {"uvs", &rb_config::uvs, &SceneFacts::n_uvs, false, {RB_ERR_INVALID_UVS, "Invalid UVs"}, {RB_ERR_UNSUPPORTED_DELETE, "not yet implemented: Implement UVs Deletion"}},
    {"meshes", &rb_config::meshes, &SceneFacts::n_meshes, false, {RB_ERR_INVALID_MESHES, "Invalid Meshes"}, {RB_ERR_UNSUPPORTED_DELETE, "not yet implemented: Implement meshes Deletion"}},
    {"lights", &rb_config::lights, &SceneFacts::n_lights, false, {RB_ERR_INVALID_LIGHTS, "Invalid Lights"}, {RB_ERR_UNSUPPORTED_DELETE, "not yet implemented: Implement lights Deletion"}},
    {"bvh_nodes", &rb_config::bvh_nodes, &SceneFacts::n_nodes, true, kNoRefusal, kNoRefusal},
    {"bvh_indices", &rb_config::bvh_indices, &SceneFacts::n_indices, true, kNoRefusal, kNoRefusal},
    {"bvh_triangles", &rb_config::bvh_triangles, &SceneFacts::n_tris, true, kNoRefusal, kNoRefusal},
    {"textures", &rb_config::textures, &SceneFacts::n_tex, false, {RB_ERR_INVALID_TEXTURES, "Invalid Textures"}, {RB_ERR_UNSUPPORTED_DELETE, "not yet implemented: Implement textures Deletion"}},
};
inline const rb_field& field_of(const rb_config* c, Field f) { return c->*kFields[f].member; }
inline bool has_data(const rb_field& f) { return f.change == RB_CREATE || f.change == RB_UPDATE; }

// ---- the plan of one update.  Together with the fields' pointers and counts in the caller's rb_config it holds everything
// the engine needs in order to act without deciding again.
enum class Act : uint8_t { None, Take, Delete };
enum class OwnTree : uint8_t { Keep, Rebuild, Empty };   // an engine that builds the tree itself: what the triangles field means for it
struct UpdatePlan {
    Act act[kFieldCount] = {};       // [kUniforms]: Take or None
    uint32_t len[kFieldCount] = {};  // the length the scene sees after the update: arrayLength(), an empty vector's one element included
    bool resize = false;             // the taken uniforms name another resolution
    ShardLayout frame;               // the rows of the taken uniforms' frame
    OwnTree own_tree = OwnTree::Keep;
    uint32_t bvh_stack = 0, max_mesh_index = 0;
    // the facts of these names at the end of the update
    uint32_t last_change_spheres = RB_KEEP, last_change_nodes = RB_KEEP, last_change_tris = RB_KEEP, last_spheres_sent = 0;
    bool have_uniforms = false;
};

inline int refuse(std::string& why, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
inline int refuse(std::string& why, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    why = buf;
    return code;
}

// tags and pointers of every field, then the uniforms' count
inline int check_tags(const rb_config* cfg, std::string& why) {
    if (!cfg) return refuse(why, RB_ERR_NULL_ARGUMENT, "config is NULL");
    for (const FieldDesc& d : kFields) {
        const rb_field& f = cfg->*d.member;
        if (f.change > RB_DELETE) return refuse(why, RB_ERR_NULL_ARGUMENT, "%s: bad change tag %u", d.name, f.change);
        if (has_data(f) && f.count > 0 && !f.ptr) return refuse(why, RB_ERR_NULL_ARGUMENT, "%s: count %zu with NULL pointer", d.name, f.count);
    }
    if (has_data(cfg->uniforms) && cfg->uniforms.count != 1)
        return refuse(why, RB_ERR_INVALID_UNIFORMS, "uniforms: expected exactly one rb_uniforms, got %zu", cfg->uniforms.count);
    return RB_OK;
}

// RenderConfig::validate_init -- render_config.rs:163-185
inline int check_first_config(const rb_config* cfg, std::string& why) {
    for (const FieldDesc& d : kFields)
        if (d.not_create.code && (cfg->*d.member).change != RB_CREATE) return refuse(why, d.not_create.code, "%s", d.not_create.text);
    return RB_OK;
}

// RenderConfig::validate -- render_config.rs:187-268: per field its values where it carries data, else its refused Delete
inline int check_values(const rb_config* cfg, std::string& why) {
    for (uint32_t i = 0; i < kFieldCount; ++i) {
        const FieldDesc& d = kFields[i];
        const rb_field& f = cfg->*d.member;
        if (f.change == RB_DELETE && d.del.code) return refuse(why, d.del.code, "%s", d.del.text);
        if (!has_data(f)) continue;
        switch (static_cast<Field>(i)) {
            case kUniforms: {
                const rb_camera& cam = static_cast<const rb_uniforms*>(f.ptr)->camera;
                if (!(cam.pane_distance >= 0.0f && cam.pane_distance <= 100.0f))
                    return refuse(why, RB_ERR_PANE_DISTANCE_OUT_OF_BOUNDS, "Pane-Distance is out of bounds");
                if (!(cam.pane_width >= 0.0f && cam.pane_width <= 1000.0f))
                    return refuse(why, RB_ERR_PANE_WIDTH_OUT_OF_BOUNDS, "Pane-Distance is out of bounds");  // sic, :631-633
                const float* dir = cam.dir;
                const float len_sq = dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2];
                if (len_sq < 1.1920929e-07f) return refuse(why, RB_ERR_INVALID_CAMERA_DIRECTION, "Invalid camera direction");
                break;
            }
            case kSpheres: {
                const rb_sphere* s = static_cast<const rb_sphere*>(f.ptr);
                for (size_t k = 0; k < f.count; ++k)
                    if (s[k].radius <= 0.0f) return refuse(why, RB_ERR_INVALID_SPHERES, "Invalid Spheres");
                break;
            }
            case kUvs:
                if (f.count % 2 != 0) return refuse(why, RB_ERR_INVALID_UVS, "Invalid UVs");
                break;
            case kLights: {
                const rb_point_light* l = static_cast<const rb_point_light*>(f.ptr);
                for (size_t k = 0; k < f.count; ++k)
                    if (l[k].radius <= 0.0f) return refuse(why, RB_ERR_INVALID_LIGHTS, "Invalid Lights");
                break;
            }
            default: break;
        }
    }
    return RB_OK;
}

// What an update does with one field.  `first` = the engine's first update (gpu_wrapper.rs:117-163: only Create is acted
// on); otherwise :165-294: Update and Delete act, Create only for a BVH field ("Create not allowed after initialization").
inline Act action_of(Field f, uint32_t change, bool first) {
    if (first) return change == RB_CREATE ? Act::Take : Act::None;
    if (change == RB_UPDATE) return Act::Take;
    if (change == RB_DELETE) return f == kUniforms ? Act::None : Act::Delete;
    if (change == RB_CREATE) return kFields[f].bvh ? Act::Take : Act::None;
    return Act::None;
}

// The plan of `cfg` on an engine in state `sc`, or the refusal: an RB_ERR_* with its text in `why` (then `pl` means nothing).
// Order: check_tags; check_first_config or check_values; the tree the kernels would walk; the triangles' meshes; the
// textures; the frame.  Passes over field data: one per field that has a rule above, one over the triangles for the largest
// mesh index, one for non-finite vertices where the engine builds the tree, one over the nodes (bvh_validate) and the leaf ranges.
inline int plan_update(const SceneFacts& sc, const rb_config* cfg, UpdatePlan& pl, std::string& why) {
    if (const int rc = check_tags(cfg, why)) return rc;
    const bool first = !sc.initialized;
    if (const int rc = first ? check_first_config(cfg, why) : check_values(cfg, why)) return rc;
    pl = UpdatePlan{};
    uint64_t len[kFieldCount] = {};
    for (uint32_t i = 0; i < kFieldCount; ++i) {
        const rb_field& f = cfg->*kFields[i].member;
        const Act a = pl.act[i] = action_of(static_cast<Field>(i), f.change, first);
        const uint64_t n = a == Act::Take ? f.count : 0;
        // an empty vector still has one element (create_storage_buffer, buffers.rs:232-249), which the counted fields' counts hide;
        // delete_lights creates a 4-byte buffer (buffers.rs:389-391): arrayLength() == 0
        const bool one_if_empty = i == kIndices || (i == kLights && a == Act::Take);
        len[i] = a == Act::None ? (kFields[i].len ? sc.*kFields[i].len : 1u) : one_if_empty ? std::max<uint64_t>(n, 1) : n;
    }
    const rb_field &f_nodes = cfg->bvh_nodes, &f_tris = cfg->bvh_triangles;
    const rb_uniforms* u = pl.act[kUniforms] == Act::Take ? static_cast<const rb_uniforms*>(cfg->uniforms.ptr) : nullptr;
    // ---- the tree the kernels would walk
    const rb_bvh_node* nodes = sc.host_nodes.data();
    len[kNodes] = sc.host_nodes.size();
    TreeSkeleton own;   // RB_FLAG_BUILD_TREE: the tree the engine will build -- its shape follows from the triangle count
    if (sc.own_tree && (f_nodes.change != RB_KEEP || cfg->bvh_indices.change != RB_KEEP))
        return refuse(why, RB_ERR_INVALID_BVH, "the engine builds the tree itself (RB_FLAG_BUILD_TREE): bvh_nodes and bvh_indices must be Keep");
    if (sc.own_tree && pl.act[kTriangles] != Act::None) pl.own_tree = pl.act[kTriangles] == Act::Take ? OwnTree::Rebuild : OwnTree::Empty;
    if (pl.own_tree == OwnTree::Rebuild) {
        if (f_tris.count >= (1ull << 31)) return refuse(why, RB_ERR_INVALID_BVH, "too many triangles");
        const size_t bad = first_non_finite(static_cast<const rb_gpu_triangle*>(f_tris.ptr), f_tris.count);
        if (bad < f_tris.count) return refuse(why, RB_ERR_INVALID_BVH, "triangle %zu has a non-finite vertex coordinate", bad);
        bvh_skeleton(f_tris.count, own);
        nodes = own.nodes.data();
        len[kNodes] = own.nodes.size();
        len[kIndices] = std::max<uint64_t>(f_tris.count, 1);
    } else if (pl.own_tree == OwnTree::Empty) {
        len[kNodes] = 0;
        len[kIndices] = 1;
    } else if (pl.act[kNodes] == Act::Take) {
        nodes = static_cast<const rb_bvh_node*>(f_nodes.ptr);
        if (f_nodes.count >= (1ull << 31)) return refuse(why, RB_ERR_INVALID_BVH, "too many BVH nodes");
        len[kNodes] = f_nodes.count;
    } else if (pl.act[kNodes] == Act::Delete) {
        len[kNodes] = 0;
    }
    if (len[kIndices] >= (1ull << 31)) return refuse(why, RB_ERR_INVALID_BVH, "too many BVH indices");
    pl.bvh_stack = sc.bvh_stack;
    if (const uint32_t n_nodes = static_cast<uint32_t>(len[kNodes])) {
        std::string fault;
        if (!bvh_validate(nodes, n_nodes, kStackDepth, fault, &pl.bvh_stack)) return refuse(why, RB_ERR_INVALID_BVH, "%s", fault.c_str());
        for (uint32_t i = 0; i < n_nodes; ++i) {
            const rb_bvh_node& n = nodes[i];
            if (n.primitive_count > 0 && static_cast<uint64_t>(n.first_primitive) + n.primitive_count > len[kIndices])
                return refuse(why, RB_ERR_INVALID_BVH, "leaf %u covers [%u, +%u) of %llu bvh_indices", i, n.first_primitive, n.primitive_count,
                              static_cast<unsigned long long>(len[kIndices]));
        }
    }
    // ---- every triangle's material must exist (shader.wgsl:370 reads meshes[tri.mesh_index])
    pl.max_mesh_index = sc.max_mesh_index;
    if (pl.act[kTriangles] == Act::Take) {
        const rb_gpu_triangle* t = static_cast<const rb_gpu_triangle*>(f_tris.ptr);
        pl.max_mesh_index = 0;
        for (size_t i = 0; i < f_tris.count; ++i) pl.max_mesh_index = std::max(pl.max_mesh_index, t[i].mesh_index);
        if (f_tris.count >= (1ull << 31)) return refuse(why, RB_ERR_INVALID_BVH, "too many triangles");
    } else if (pl.act[kTriangles] == Act::Delete) {
        pl.max_mesh_index = 0;
    }
    const uint32_t color_hash = u ? u->color_hash_enabled : sc.uniforms.color_hash_enabled;
    if (len[kTriangles] > 0 && color_hash == 0 && pl.max_mesh_index >= len[kMeshes])
        return refuse(why, RB_ERR_INVALID_MESHES, "a triangle references mesh %u of %llu", pl.max_mesh_index, static_cast<unsigned long long>(len[kMeshes]));
    // ---- textures and the frame
    if (pl.act[kTextures] == Act::Take) {
        const rb_texture* t = static_cast<const rb_texture*>(cfg->textures.ptr);
        for (size_t i = 0; i < cfg->textures.count; ++i) {
            if (t[i].width == 0 || t[i].height == 0) return refuse(why, RB_ERR_INVALID_TEXTURES, "texture %zu is empty", i);
            if (!t[i].rgba_data) return refuse(why, RB_ERR_INVALID_TEXTURES, "texture %zu has no data", i);
        }
    }
    if (u) {
        pl.frame = sc.layout(u->height);
        if (static_cast<uint64_t>(u->width) * pl.frame.padded >= (1ull << 31))
            return refuse(why, RB_ERR_INVALID_UNIFORMS, "frame of %u x %u pixels is too large", u->width, u->height);
        pl.resize = u->width != sc.width || u->height != sc.height;
    }
    for (uint32_t i = 0; i < kFieldCount; ++i) pl.len[i] = static_cast<uint32_t>(len[i]);
    // ---- self.rc = new_rc (:298): the counts are patched from, and width()/height()/update_uniforms panic unless it carried
    // Create/Update uniforms in, the *latest* config (:303-329,470-495)
    pl.have_uniforms = has_data(cfg->uniforms);
    pl.last_change_spheres = cfg->spheres.change;
    // the vector's length where it was acted on is the buffer's; where a Create was ignored it is the count all the same (:476)
    pl.last_spheres_sent = has_data(cfg->spheres) ? static_cast<uint32_t>(std::min<size_t>(cfg->spheres.count, 0xFFFFFFFFu)) : 0xFFFFFFFFu;
    pl.last_change_nodes = sc.own_tree ? f_tris.change : f_nodes.change;
    pl.last_change_tris = f_tris.change;
    return RB_OK;
}

// ---- the only places where facts change.  A field's facts change when its buffer has been written (the uniforms': when
// the frame has its size), the own tree's when it has been built, the rest at the end of the update: an update that fails
// half-way on the device leaves facts that describe the buffers as far as they got.

// the flat kernels' facts of a field that is taken or deleted.  A deleted field has no element a launch reads: vacuously true.
// (An empty lights vector leaves one zero-filled light, texture index 0, which the kernels scan like any other.)
inline void commit_trace_facts(SceneFacts& sc, const UpdatePlan& pl, const rb_config* cfg, Field f) {
    const bool take = pl.act[f] == Act::Take;
    const rb_field& fd = field_of(cfg, f);
    switch (f) {
        case kMeshes: sc.untex_meshes = !take || untextured(static_cast<const rb_mesh*>(fd.ptr), fd.count); break;
        case kSpheres: sc.untex_spheres = !take || untextured(static_cast<const rb_sphere*>(fd.ptr), fd.count); break;
        case kLights: sc.untex_lights = !take || (fd.count > 0 && untextured(static_cast<const rb_point_light*>(fd.ptr), fd.count)); break;
        default: return;
    }
    sc.no_uv = sc.untex_meshes && sc.untex_spheres;
}

inline void commit_field(SceneFacts& sc, const UpdatePlan& pl, const rb_config* cfg, Field f) {
    if (f == kUniforms) {
        if (pl.act[f] == Act::Take) {
            sc.uniforms = *static_cast<const rb_uniforms*>(cfg->uniforms.ptr);
            sc.width = sc.uniforms.width, sc.height = sc.uniforms.height;
            sc.local_rows = pl.frame.whole_rows, sc.padded_rows = pl.frame.padded;
        }
        sc.have_uniforms = pl.have_uniforms;
        return;
    }
    if (pl.act[f] == Act::None) return;
    sc.*kFields[f].len = pl.len[f];
    commit_trace_facts(sc, pl, cfg, f);
    if (f == kNodes) {
        const rb_bvh_node* src = static_cast<const rb_bvh_node*>(cfg->bvh_nodes.ptr);
        sc.host_nodes.assign(src, src + pl.len[f]);
    }
}

// the tree an engine built over n_tris triangles (OwnTree::Rebuild; OwnTree::Empty: none over 0), its boxes included
inline void commit_own_tree(SceneFacts& sc, std::vector<rb_bvh_node>&& nodes, size_t n_tris) {
    sc.n_nodes = static_cast<uint32_t>(nodes.size());
    sc.n_indices = static_cast<uint32_t>(std::max<size_t>(n_tris, 1));
    sc.host_nodes = std::move(nodes);
}

inline void commit_end(SceneFacts& sc, const UpdatePlan& pl) {
    sc.last_change_spheres = pl.last_change_spheres;
    sc.last_spheres_sent = pl.last_spheres_sent;
    sc.last_change_nodes = pl.last_change_nodes;
    sc.last_change_tris = pl.last_change_tris;
    sc.bvh_stack = pl.bvh_stack;
    sc.max_mesh_index = pl.max_mesh_index;
    sc.initialized = true;
}

// update_uniforms count patch-up -- gpu_wrapper.rs:475-495: Create/Update overwrite the count with the
// vector length, Delete zeroes it, Keep leaves the caller's value (clamped to the buffer here so that a
// stale count cannot read out of bounds; the WGSL relies on robust buffer access for that).
inline uint32_t patch_count(uint32_t change, uint32_t given, uint32_t len) {
    if (change == RB_CREATE || change == RB_UPDATE) return len;
    if (change == RB_DELETE) return 0u;
    return std::min(given, len);
}
// the three patched counts of the current facts
inline uint32_t spheres_count(const SceneFacts& sc) { return patch_count(sc.last_change_spheres, sc.uniforms.spheres_count, std::min(sc.n_spheres, sc.last_spheres_sent)); }
inline uint32_t node_count(const SceneFacts& sc) { return patch_count(sc.last_change_nodes, sc.uniforms.bvh_node_count, sc.n_nodes); }
inline uint32_t triangle_count(const SceneFacts& sc) { return patch_count(sc.last_change_tris, sc.uniforms.bvh_triangle_count, sc.n_tris); }

}  // namespace rb
