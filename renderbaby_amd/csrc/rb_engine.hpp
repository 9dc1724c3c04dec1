// rb_engine.hpp -- the engine's state, shared by the runtime (rb_runtime.cpp), the acceleration structures it builds
// (rb_accel.cpp), the queries over them (rb_queries.cpp) and the frame's post-processing (rb_frame.cpp).  Host code only: not
// part of the ABI, and no .hip file includes it.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "rb_color_plan.hpp"
#include "rb_internal.hpp"
#include "rb_rccl.hpp"
#include "rb_stage_timer.hpp"
#include "rb_tri_filter.hpp"
#include "rb_update_plan.hpp"

namespace rb {

template <typename T>
struct DevBuf {
    T* ptr = nullptr;
    size_t count = 0;     // elements allocated
    ~DevBuf() { release(); }
    void release() {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        count = 0;
    }
    hipError_t resize(size_t n) {
        if (n == count && ptr) return hipSuccess;
        release();
        if (n == 0) return hipSuccess;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&ptr), n * sizeof(T));
        if (e == hipSuccess) count = n;
        return e;
    }
    void adopt(T* p, size_t n) {   // take over an allocation made elsewhere (rb_build.hip)
        release();
        ptr = p;
        count = n;
    }
    // scratch that is sized per launch: keep an allocation that is large enough and not wastefully so
    bool serves(size_t n) const { return ptr && n <= count && count <= 4 * std::max<size_t>(n, 1); }
    hipError_t reserve(size_t n) { return serves(n) ? hipSuccess : resize(n); }
};

// One frame: the accumulation (vec4<f32> per pixel: sum of radiance, sample count) and the packed RGBA8
// image the kernels derive from it.  `done` is recorded after the launches that produced this slot.
struct FrameSlot {
    DevBuf<float> accum;
    DevBuf<uint32_t> rgba;
    hipEvent_t done = nullptr;
};

// ---- the acceleration structures (rb_accel.cpp): each keeps its device buffers, its header and one build record: which
// builder made it and how long that took (rb_*_builder).  An empty name means "not built".
struct BuildRecord {
    const char* builder = "";
    float ms = 0.0f;
    bool built() const { return builder[0] != '\0'; }
};

struct SphereAccel {   // the spheres' tree: "device-median" | "host-median"
    DevBuf<SphereNode4> nodes;
    DevBuf<float> leaf;
    DevBuf<uint32_t> id;
    uint32_t root = 0, depth = 0;   // depth: the stack entries of its walk
    BuildRecord rec;
};

struct ChunkAccel {    // the chunked walk's tree (ChunkTree): "device" | "host"
    DevBuf<ChunkNode> nodes;
    DevBuf<float> a, b, c;
    DevBuf<uint32_t> rank_slot;
    DevBuf<uint32_t> pos_slot, pos_rank;   // chunk order -> slot / rank: read by the gather at build time, kept for rb_debug_engine_chunk_tree
    size_t n_nodes = 0;
    uint32_t root = 0, depth = 0;
    BuildRecord rec;
};

struct OwnAccel {      // the library's own triangle tree (walk mode "fast"): "device-ploc" | "device-lbvh" | "host-sah"
    DevBuf<SphereNode> nodes;
    DevBuf<PrepTri> tris;
    DevBuf<uint32_t> slots, slot_meta, ref_parent, stack_overflow;
    DevBuf<GrazeNode> gnodes;
    DevBuf<uint32_t> gslots;
    DeviceTreeInfo info{};   // root, depth, margin, root_amax and the mesh bounds, whichever builder ran
    BuildRecord rec;
};

// The mesh walks an engine may build, from its options alone (mesh_walks); the mesh decides the rest.
struct MeshWalks {
    bool host_mesh = false;   // not RB_FLAG_REFERENCE_WALK: a host builder may need the host's copy of the mesh
    bool chunk = false;       // the chunked walk's tree, tried first
    bool own_named = false;   // a flag names the library's own tree: wanted at any size (unless the reference walk is named) ...
    bool own(uint32_t n_tris) const { return host_mesh && (own_named || n_tris >= kOwnTreeDefaultMinTriangles); }  // ... else from this size up
};

}  // namespace rb

struct rb_engine {
    std::mutex mu;
    mutable std::mutex err_mu;       // guards `error` for the const getters (rb_get_size, rb_last_error)
    mutable std::string error;
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr;   // read-backs into page-locked caller memory
    // A launch group in two colour parts (dispatch): odd trace launches go to `trace_stream`, so that a launch fills the wave slots
    // the one before it vacates, and every k_accumulate to `accum_stream`, underneath the next launch's trace.  Both non-blocking,
    // both joined into `stream` before a dispatch returns, so nothing else in the library needs to know of them.
    hipStream_t accum_stream = nullptr;
    hipStream_t trace_stream = nullptr;
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;
    hipEvent_t ev_top = nullptr;                          // the top of a launch group on `stream` (no timing)
    hipEvent_t ev_traced[2] = {nullptr, nullptr};         // per colour part: its trace launch is over (no timing)
    hipEvent_t ev_accumulated[2] = {nullptr, nullptr};    // per colour part: its accumulate is over, the part is free (no timing)
    std::vector<hipEvent_t> ev_pool;   // per launch chunk: trace begin, trace end, accumulate begin, accumulate end
    uint32_t ev_used = 0;
    const char* last_kernel_name = "";
    rb_options opt{};

    rb::SceneFacts sc;               // what rb_update decides on (rb_update_plan.hpp): lengths, uniforms, frame size; changed by commit_* only
    bool scene_valid = false;        // the buffers hold a scene that passed plan_update (set by the last update)
    bool trace_uv = false;           // RB_TRACE_UV=1 when the engine was made: KParams::no_uv stays 0 (the kernels with u, v)
    uint32_t last_trace_form = 0;    // the last render launch's LaunchInfo::trace_form (rb_debug_trace_form)
    // The triangle sift of a single-node tree (rb_tri_filter.hpp; DESIGN.md section 4, "The triangle sift").  The table is remade
    // with the prepared triangles (ensure_prepared), the region per launch (make_params): it follows the camera and the spheres.
    bool tri_filter = true;          // RB_TRI_FILTER=0 when the engine was made: KParams::sift stays 0 (k_trace_flat as before)
    rb::SiftTable sift_table;        // empty: no table (more than one node, a list beyond kSiftMaxSlots, nothing to reject)
    rb::DevBuf<rb::SiftGroup> sift_groups;
    float sph_box[6] = {0, 0, 0, 0, 0, 0};   // lo, hi of the uploaded spheres (all of them, whatever the patched count)
    bool sph_box_any = false;
    rb_progressive prh{};            // gpu_wrapper.rs:19-53
    bool iter_initialized = false;   // RaytracerFrameIterator::initialized (lib.rs:131)
    uint32_t iter_passes_per_frame = 1;  // rb_iter_set_passes_per_frame (1 = the reference's one frame per pass)

    bool prep_dirty = true;
    uint32_t prep_tri_count = 0xFFFFFFFFu;  // uniforms.bvh_triangle_count (patched) the prepared triangles were made for

    rb::DevBuf<rb_sphere> spheres;
    rb::DevBuf<float> sph_scan;      // float4 {centre, radius * radius} per sphere of `spheres`, remade whenever those are taken (KParams::sph_scan)
    rb::DevBuf<rb_point_light> lights;
    rb::DevBuf<rb_mesh> meshes;
    rb::DevBuf<rb_bvh_node> nodes;
    rb::DevBuf<uint32_t> indices;
    rb::DevBuf<rb_gpu_triangle> tris;
    rb::DevBuf<rb::PrepTri> ptris;
    rb::DevBuf<rb::PrepTriShade> pshade;
    rb::DevBuf<float> uvs;
    rb::DevBuf<uint32_t> tex_data;
    rb::DevBuf<rb_texture_info> tex_info;
    rb::DevBuf<float> srgb_lut;
    rb::FrameSlot slot[2];           // slot[cur] holds the committed frame
    int cur = 0;
    bool spec_valid = false;         // slot[1 - cur] holds passes [spec_first, +spec_n) run ahead on top of slot[cur]
    uint32_t spec_first = 0, spec_n = 0;
    rb::DevBuf<unsigned long long> counters;
    rb::DevBuf<uint32_t> queue;      // two sets of rb::kQueueWords: two trace launches may be in flight (dispatch)
    rb::SphereAccel sph;
    rb::ChunkAccel chunk;
    rb::OwnAccel own;
    rb::BuildRecord tree;            // who made the reference-layout tree (`nodes`, `indices`): "device" | "host" (RB_FLAG_BUILD_TREE*) | "caller"
    // The host's copy of the mesh, for the host builders and the checkers.  A large mesh (>= kChunkDeviceBuildMin elements: the
    // device builder's territory) is NOT copied at rb_update -- a second 88 MB in host memory cost C5's update 10 of its 14 ms --
    // but fetched back from the device buffer if a host builder turns out to be needed after all (ensure_host_mesh).
    std::vector<rb_gpu_triangle> host_tris;
    std::vector<uint32_t> host_indices;
    size_t host_tri_len = 0, host_index_len = 0;   // what the vectors hold, or would hold (0: the engine keeps no copy)
    bool host_tris_stale = false, host_indices_stale = false;
    bool stack_depth_covers = true;    // set with KParams::stack_depth: every walk in use fits its LDS column
    rb::DevBuf<float> colors;        // RB_KERNEL_STREAM: float4 per (pixel, sample) of one launch chunk, times the parts of the plan
    size_t color_part_floats = 0;    // part k of the last reservation starts at colors.ptr + k * color_part_floats
    uint64_t color_budget = 0;       // bytes `colors` may take (0 = ask the device at the next dispatch)

    // closest-hit queries (rb_cast_rays / rb_render_hits / rb_pick): scratch for one piece of at most rb::kQueryPiece rays (a
    // frame piece: whole 8-row bands, so at least 8 x width records), the kernel and the kernel time of the last one; nothing of a render is touched
    rb::DevBuf<rb_ray> q_rays;
    rb::DevBuf<rb_hit> q_hits;
    rb::DevBuf<rb_surface> q_surf;
    rb::DevBuf<float> q_tmax;        // rb_occluded: the piece's bounds and its result bytes
    rb::DevBuf<uint8_t> q_occl;
    rb::DevBuf<float> rad_colors;    // rb_trace_rays: float4 per (ray, sample) of one piece, the piece's ids and sums, the queue word
    rb::DevBuf<uint32_t> rad_seeds, rad_queue;
    rb::DevBuf<rb_radiance> rad_out;
    rb::DevBuf<rb_surfel> hemi_surfels;   // rb_trace_hemisphere / rb_openness_hemisphere: the piece's surfels and its counts
    rb::DevBuf<rb_openness> hemi_open;
    rb::DevBuf<rb_probe> probe_pos;       // rb_bake_probes: the piece's probes and its SH9 sums
    rb::DevBuf<rb_sh9> probe_out;
    rb::DevBuf<rb_probe_depth> depth_out; // rb_bake_probe_depth: the piece's maps (its records and hits: q_rays, q_hits)
    // direct light (rb_scene_emitters / rb_direct_light): the emitter table of the scene of the last
    // accepted update (made by the first call that needs it after it) with its length on both sides, the compaction's
    // scratch, and a caller's table as the host form stages it
    rb::DevBuf<rb_emitter> emit_table, emit_given;
    rb::DevBuf<uint32_t> emit_count;
    rb::DevBuf<unsigned char> emit_work;
    uint32_t emit_n = 0;
    bool emit_valid = false;
    // the weighted pick (rb_scene_emitter_cdf / rb_direct_light_cdf): the scene's table by power, made
    // by the first call that needs it after the emitter table and kept as long; the table by power of a caller's emitters and
    // a caller's own table as the host form stages it; the build's scratch
    rb::DevBuf<uint32_t> emit_cdf, emit_cdf_given;
    rb::DevBuf<unsigned char> emit_cdf_work;
    bool emit_cdf_valid = false;
    // the pick per grid cell (rb_emitter_grid_cdf_device / rb_direct_light_grid): the tables of one call
    // -- made for it, or a caller's as the host form stages them -- and the build's scratch.  The engine keeps no grid.
    rb::DevBuf<uint32_t> emit_grid_tables;
    rb::DevBuf<unsigned char> emit_grid_work;
    // the host form's tally of rb_direct_light_grid_tally between its upload and its download (section 25); the engine keeps none
    rb::DevBuf<rb_grid_tally> emit_grid_tally;
    // lightmap texels made on the device (rb_lightmap_surfels_device / rb_bake_lightmap*): the triangles
    // prepared in triangle order, the cover pass's scratch, and what a bake keeps between its stages
    rb::DevBuf<rb::PrepTri> lm_ptris;
    rb::DevBuf<rb::PrepTriShade> lm_pshade;
    rb::DevBuf<uint32_t> lm_iota, lm_owners;
    rb::DevBuf<unsigned char> lm_work;
    rb::DevBuf<rb_surfel> lm_surfels;
    rb::DevBuf<rb_radiance> lm_sums;
    rb::DevBuf<float> lm_rgba[2];
    // the stage times of the most recent query: reset by every query's prologue, the lightmap's two by
    // a lightmap call alone
    rb::StageTimer t_query;          // a query's kernels (rb_last_query_ms)
    rb::StageTimer t_generator;      // a pair round every piece's generator (rb_last_camera_rays_ms)
    rb::StageTimer t_sh, t_depth;    // ... round every piece's projection (rb_last_probe_project_ms, rb_last_probe_depth_project_ms)
    rb::StageTimer t_lm_surfels, t_lm_resolve;   // the lightmap's first and last stage (rb_last_lightmap_ms)
    const char* last_query_kernel_name = "";

    // the denoiser (rb_denoise*): the guide planes of the scene and camera of the last accepted update (made
    // by the first denoise after it), the two colour buffers the iterations ping-pong between, staging for host outputs, and
    // timers of its own: like a query it moves neither the work counters nor the timing of a launch group
    // (two sets of planes: the history of section 22 keeps the set its frame was made with while the next update's guides are
    // built into the other one; dn_set is the current one)
    rb::DevBuf<float> dn_nt[2], dn_pc[2], dn_al[2];
    int dn_set = 0;
    bool dn_guides_valid = false;
    rb::DevBuf<float> dn_r[2], dn_linear;
    rb::DevBuf<uint32_t> dn_rgba;
    rb::StageTimer t_guides, t_filter;   // the guide build and the filter of the most recent denoise (rb_last_denoise_ms)

    // temporal reprojection (rb_denoise_history): the history H -- the frame records F of the most recent
    // call, the set of guide planes they belong to (hist_set), their view and size --, and the base B: H carried into the current
    // guides, made by the first call after an accepted update, so that repeated calls do not count their own samples twice
    rb::DevBuf<float> hist_frame, hist_base;
    int hist_set = 0;
    rb::DevBuf<float> rp_planes;   // rb_reproject_device: the six planes of its two guide arrays
    rb_view hist_view{};
    uint32_t hist_w = 0, hist_h = 0;
    bool hist_valid = false, hist_base_valid = false;
    rb::StageTimer t_history;   // REPROJECT (if made) and MERGE of the most recent rb_denoise_history (rb_last_reproject_ms)

    rb_stats stats{};
    float last_dispatch_ms = 0.0f;
    uint32_t last_launches = 0;
    bool timing_pending = false;

    // ---- several devices behind one handle (rb_create_multi): this engine only coordinates; every part is a
    // complete engine for one shard on one device.  Or one process per device (rb_comm_init_rank): this engine
    // is shard `opt.shard_rank` and `net` holds its communicator.
    std::vector<std::unique_ptr<rb_engine>> parts;
    rb::Gather net;
};

namespace rb {

// sets the error text of `e` (of the failing create when e is NULL) and returns `code`
int fail(const rb_engine* e, int code, const char* fmt, ...);

#define HIP_TRY(e, call)                                                                          \
    do {                                                                                          \
        hipError_t _st = (call);                                                                  \
        if (_st != hipSuccess)                                                                    \
            return rb::fail((e), RB_ERR_DEVICE, "%s failed: %s", #call, hipGetErrorString(_st));  \
    } while (0)

// create_storage_buffer -- buffers.rs:232-249: an empty slice still allocates one
// zero-filled element (wgpu zero-initialises), so arrayLength() is 1.
// The copy is queued on the engine's stream from caller memory: every path that calls this ends in
// update_locked's hipStreamSynchronize (or an earlier one) before the caller gets its buffers back.
template <typename T>
int upload(rb_engine* e, DevBuf<T>& buf, const void* src, size_t count, bool pad_empty) {
    const size_t alloc = (count == 0 && pad_empty) ? 1 : count;
    HIP_TRY(e, buf.resize(alloc));
    if (count > 0) {
        HIP_TRY(e, hipMemcpyAsync(buf.ptr, src, count * sizeof(T), hipMemcpyHostToDevice, e->stream));
    } else if (alloc > 0) {
        HIP_TRY(e, hipMemsetAsync(buf.ptr, 0, alloc * sizeof(T), e->stream));
    }
    return RB_OK;
}

inline bool is_group(const rb_engine* e) { return !e->parts.empty(); }
inline void set_device(const rb_engine* e) { (void)hipSetDevice(e->device); }
inline uint32_t kernel_of(const rb_options& opt) { return opt.kernel ? opt.kernel : RB_KERNEL_STREAM; }

// ---- rb_runtime.cpp, for rb_queries.cpp and rb_frame.cpp (hidden: the library's dynamic symbols stay what they were)
#define RB_HIDDEN __attribute__((visibility("hidden")))
RB_HIDDEN int require_ready(rb_engine* e);      // the engine holds a scene that a launch may read, or the refusal
RB_HIDDEN int ensure_prepared(rb_engine* e);    // the prepared triangles and the mesh walk's tree of the current scene
RB_HIDDEN KParams make_params(rb_engine* e, uint32_t first_pass, uint32_t n_passes, int src, int dst);
RB_HIDDEN void copy_error(rb_engine* g, const rb_engine* part);
#undef RB_HIDDEN

// ---- rb_accel.cpp
constexpr uint32_t kBuildTreeFlags = RB_FLAG_BUILD_TREE | RB_FLAG_BUILD_TREE_HOST;          // the engine builds the reference-layout tree
constexpr uint32_t kOwnTreeFlags = RB_FLAG_FAST_BVH | RB_FLAG_DEVICE_BVH | RB_FLAG_HOST_BVH;  // they name the own tree as the walk
inline bool builds_tree(const rb_options& opt) { return (opt.flags & kBuildTreeFlags) != 0u; }
MeshWalks mesh_walks(const rb_options& opt);
bool host_copy_can_wait(const rb_engine* e, size_t n);   // may a mesh field of n elements leave its host copy to ensure_host_mesh?
int ensure_host_mesh(rb_engine* e);
int build_sphere_bvh(rb_engine* e, const rb_sphere* s, size_t n);              // Take / Delete of spheres
int build_engine_tree(rb_engine* e, const rb_gpu_triangle* src, size_t n);     // RB_FLAG_BUILD_TREE: Take / Delete of triangles
int build_chunk_tree(rb_engine* e, uint32_t tri_count);   // ensure_prepared, when wanted (tri_count: the patched count)
int build_own_tree(rb_engine* e, uint32_t tri_count);
uint32_t accel_params(const rb_engine* e, KParams& p);     // every structure's KParams fields; returns the stack entries needed

}  // namespace rb
