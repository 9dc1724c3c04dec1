// rb_accel.cpp -- the engine's acceleration structures: the sphere tree, the reference-layout tree (RB_FLAG_BUILD_TREE), the
// chunked walk's tree and the library's own triangle tree.  Each has one build function, one build record and its own KParams
// fields.  Which mesh walks an engine may build follows from its options (mesh_walks); which builder runs, from device_builder.
#include <chrono>
#include <cstddef>
#include <cstring>

#include "rb_engine.hpp"

namespace rb {
namespace {

using Clock = std::chrono::steady_clock;
float ms_since(Clock::time_point t) { return std::chrono::duration<float, std::milli>(Clock::now() - t).count(); }

// The builder rule of every structure: the flag that forces a builder if one is set, else the device's from the structure's
// threshold up.  The frame does not depend on which builder ran.
bool device_builder(const rb_engine* e, uint32_t force_host, uint32_t force_device, bool at_threshold) {
    if (e->opt.flags & force_host) return false;
    return (e->opt.flags & force_device) != 0u || at_threshold;
}

// the chunked walk's tree over n_idx index slots: the device builder from kChunkDeviceBuildMin slots up (one block per
// reference leaf; C5's 10^6 triangles in a few ms where the host's threads take 11-15), the host's below
bool chunk_tree_on_device(const rb_engine* e, size_t n_idx) {
    return device_builder(e, RB_FLAG_CHUNK_TREE_HOST, RB_FLAG_CHUNK_TREE_DEVICE, n_idx >= kChunkDeviceBuildMin);
}

// a device array's first n elements into a host vector (synchronous)
template <typename T>
hipError_t read_back(std::vector<T>& v, const T* dev, size_t n) {
    v.resize(n);
    return hipMemcpy(v.data(), dev, sizeof(T) * n, hipMemcpyDeviceToHost);
}

// a mesh that a tree of the library's can go with: a multi-node caller tree, triangles and indices, a positive count
bool mesh_takes_tree(const rb_engine* e, uint32_t tri_count) {
    return e->sc.host_nodes.size() > 1 && e->host_tri_len > 0 && e->host_index_len > 0 && tri_count > 0;
}

// Each structure's KParams fields, and the stack entries its walk needs (0: not in use).
uint32_t params(const ChunkAccel& c, bool use, KParams& p) {
    p.chunk_nodes = use ? c.nodes.ptr : nullptr;
    p.chunk_a = c.a.ptr;
    p.chunk_b = c.b.ptr;
    p.chunk_c = c.c.ptr;
    p.chunk_rank_slot = c.rank_slot.ptr;
    p.chunk_root = c.root;
    p.chunk_n = static_cast<uint32_t>(c.rank_slot.count);
    return use ? c.depth + 1u : 0u;
}

uint32_t params(const OwnAccel& o, bool use, bool skip_second_pass, KParams& p) {
    p.fast_nodes = use ? o.nodes.ptr : nullptr;
    p.gnodes = o.gnodes.ptr;
    p.gslots = o.gslots.ptr;
    p.fast_skip_second_pass = skip_second_pass ? 1u : 0u;
    p.fast_tris = reinterpret_cast<const float*>(o.tris.ptr);
    p.fast_slots = o.slots.ptr;
    p.slot_meta = o.slot_meta.ptr;
    p.ref_parent = o.ref_parent.ptr;
    p.fast_root = o.info.root;
    p.fast_margin = o.info.margin;
    p.fast_root_amax = o.info.root_amax;
    std::memcpy(p.fast_bmin, o.info.bmin, sizeof p.fast_bmin);
    std::memcpy(p.fast_bmax, o.info.bmax, sizeof p.fast_bmax);
    p.stack_overflow = o.stack_overflow.ptr;
    return use ? std::min(o.info.depth, kStackDepth) : 0u;   // the rest spills to stack_overflow
}

uint32_t params(const SphereAccel& s, bool use, KParams& p) {
    p.sph_nodes = use ? s.nodes.ptr : nullptr;
    p.sph_leaf = s.leaf.ptr;
    p.sph_id = s.id.ptr;
    p.sph_root = s.root;
    return use ? s.depth : 0u;
}

// what a builder getter reports: a group handle answers from its first part (every part holds the same scene)
template <typename Get>
const char* report(const rb_engine* e, float* build_ms, Get get) {
    const BuildRecord r = e ? get(is_group(e) ? *e->parts[0] : *e) : BuildRecord{};
    if (build_ms) *build_ms = r.ms;
    return r.builder;
}

// The checks rb_bvh_build_canonical and rb_bvh_build_device share.  Sets *n_nodes, which follows from n_tris alone; returns
// kSizeQuery when only that size was asked (no build, no device, no look at the triangles), RB_OK to build, or an RB_ERR_*.
constexpr int kSizeQuery = -1;   // every RB_ERR_* is positive
int canonical_build_args(const rb_gpu_triangle* tris, size_t n_tris, const rb_bvh_node* nodes_out, size_t nodes_capacity, size_t* n_nodes) {
    if (!n_nodes) return RB_ERR_NULL_ARGUMENT;
    if (n_tris >= (1ull << 31)) return fail(nullptr, RB_ERR_INVALID_BVH, "too many triangles");
    *n_nodes = bvh_node_count(n_tris);
    if (!nodes_out) return kSizeQuery;
    if (n_tris > 0 && !tris) return RB_ERR_NULL_ARGUMENT;
    if (nodes_capacity < *n_nodes) return RB_ERR_INVALID_BVH;
    const size_t bad = first_non_finite(tris, n_tris);
    if (bad < n_tris) return fail(nullptr, RB_ERR_INVALID_BVH, "triangle %zu has a non-finite vertex coordinate", bad);
    return RB_OK;
}

// rb_debug_*chunk_tree: the tree's invariants checked against its mesh, then its census in out6
int check_and_count(const rb_engine* e, const char* what, const ChunkTree& t, const rb_gpu_triangle* tris, uint32_t n_tris,
                    const uint32_t* indices, uint32_t n_indices, uint64_t out6[6]) {
    std::string why;
    if (!chunk_tree_check(t, tris, n_tris, indices, n_indices, kStackDepth, why)) return fail(e, RB_ERR_INVALID_BVH, "%s: %s", what, why.c_str());
    uint64_t chunks = 0, unbounded = 0;
    for (const ChunkNode& c : t.nodes) {
        chunks += ((c.lref != kChunkNone && (c.lref & kChunkLeaf)) ? 1 : 0) + ((c.rref != kChunkNone && (c.rref & kChunkLeaf)) ? 1 : 0);
        unbounded += ((c.lref != kChunkNone && (c.lfac >> 16) == 0x7F80u) ? 1 : 0) + ((c.rref != kChunkNone && (c.rfac >> 16) == 0x7F80u) ? 1 : 0);
    }
    const uint64_t census[6] = {1, t.nodes.size(), t.pos_slot.size(), t.depth, chunks, unbounded};
    std::copy(census, census + 6, out6);
    return RB_OK;
}

// rb_debug_*own_tree / rb_debug_*sphere_tree: the header words of a tree and the capacity checks, before anything is copied.
// The ABI's node records are the library's own, field for field.
static_assert(sizeof(rb_debug_own_node) == sizeof(SphereNode) && offsetof(rb_debug_own_node, left_fa) == offsetof(SphereNode, _pad0) &&
              offsetof(rb_debug_own_node, right_fa) == offsetof(SphereNode, _pad1), "rb_debug_own_node is SphereNode");
static_assert(sizeof(rb_debug_sphere_node) == sizeof(SphereNode4) && offsetof(rb_debug_sphere_node, ref) == offsetof(SphereNode4, ref) &&
              offsetof(rb_debug_sphere_node, axes) == offsetof(SphereNode4, axes), "rb_debug_sphere_node is SphereNode4");
struct OwnTreeCopy {
    size_t n_nodes = 0, n_slots = 0, n_meta = 0;
    uint32_t root = 0, depth = 0;
    const float *bmin = nullptr, *bmax = nullptr;
};
int own_tree_header(const rb_engine* e, const OwnTreeCopy& c, const void* nodes_out, size_t nodes_capacity, const void* slots_out,
                    size_t slots_capacity, const void* slot_meta_out, size_t slot_meta_capacity, uint64_t counts3[3], uint32_t root_depth[2],
                    float bounds6[6]) {
    counts3[0] = c.n_nodes;
    counts3[1] = c.n_slots;
    counts3[2] = c.n_meta;
    root_depth[0] = c.root;
    root_depth[1] = c.depth;
    for (int a = 0; a < 3; ++a) {
        bounds6[a] = c.bmin ? c.bmin[a] : 0.0f;
        bounds6[3 + a] = c.bmax ? c.bmax[a] : 0.0f;
    }
    if (nodes_out && nodes_capacity < c.n_nodes) return fail(e, RB_ERR_INVALID_BVH, "nodes_out holds %zu of %zu nodes", nodes_capacity, c.n_nodes);
    if (slots_out && slots_capacity < c.n_slots) return fail(e, RB_ERR_INVALID_BVH, "slots_out holds %zu of %zu slots", slots_capacity, c.n_slots);
    if (slot_meta_out && slot_meta_capacity < c.n_meta)
        return fail(e, RB_ERR_INVALID_BVH, "slot_meta_out holds %zu of %zu words", slot_meta_capacity, c.n_meta);
    return RB_OK;
}
int sphere_tree_header(const rb_engine* e, size_t n_nodes, size_t n, uint32_t root, uint32_t depth, const void* nodes_out, size_t nodes_capacity,
                       const void* leaf_out, const void* id_out, size_t spheres_capacity, uint64_t counts2[2], uint32_t root_depth[2]) {
    counts2[0] = n_nodes;
    counts2[1] = n;
    root_depth[0] = root;
    root_depth[1] = depth;
    if (nodes_out && nodes_capacity < n_nodes) return fail(e, RB_ERR_INVALID_BVH, "nodes_out holds %zu of %zu nodes", nodes_capacity, n_nodes);
    if ((leaf_out || id_out) && spheres_capacity < n)
        return fail(e, RB_ERR_INVALID_BVH, "leaf_out / id_out hold %zu of %zu spheres", spheres_capacity, n);
    return RB_OK;
}

}  // namespace

MeshWalks mesh_walks(const rb_options& opt) {
    MeshWalks w;
    w.host_mesh = !(opt.flags & RB_FLAG_REFERENCE_WALK);
    w.own_named = (opt.flags & kOwnTreeFlags) != 0u;
    // the chunked walk (k_trace_chunk) is the fastest exact walk at every size measured (profiles/r03_walks.txt: 576 to
    // 1 048 578 triangles): the default; the one-pixel-per-lane dispatch shapes walk per segment
    w.chunk = kernel_of(opt) == RB_KERNEL_STREAM && ((opt.flags & RB_FLAG_CHUNK_WALK) || (w.host_mesh && !w.own_named));
    return w;
}

// large enough for the chunked walk's device builder, and no flag that sends the build to a host builder (or to the own tree,
// whose builders all start from the host's copy) anyway
bool host_copy_can_wait(const rb_engine* e, size_t n) {
    return n >= kChunkDeviceBuildMin && chunk_tree_on_device(e, n) && !mesh_walks(e->opt).own_named;
}

// The host builders and checkers read host_tris / host_indices: bring back what rb_update left on the device only.
int ensure_host_mesh(rb_engine* e) {
    if (!e->host_tris_stale && !e->host_indices_stale) return RB_OK;
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    if ((e->host_tris_stale && e->host_tri_len > e->tris.count) || (e->host_indices_stale && e->host_index_len > e->indices.count))
        return fail(e, RB_ERR_DEVICE, "a device buffer of the mesh is shorter than the mesh it was made from");
    if (e->host_tris_stale) HIP_TRY(e, read_back(e->host_tris, e->tris.ptr, e->host_tri_len));
    if (e->host_indices_stale) HIP_TRY(e, read_back(e->host_indices, e->indices.ptr, e->host_index_len));
    e->host_tris_stale = e->host_indices_stale = false;
    return RB_OK;
}

// Spheres beyond kSphereBvhThreshold get the library's own acceleration structure; the
// reference's linear scan (shader.wgsl:574-586) stays the rule for small counts.  From kSphereDeviceBuildMin spheres
// up the tree is made on the device from the copy that is already there (rb_build.hip: the same median splits, one
// segmented sort per level; 10^6 spheres in milliseconds where the host takes 0.1 s);
// either builder can be forced.
int build_sphere_bvh(rb_engine* e, const rb_sphere* s, size_t n) {
    SphereAccel& t = e->sph;
    t.rec = {};
    if (n <= kSphereBvhThreshold || n >= (1u << 27) || (e->opt.flags & RB_FLAG_NO_SPHERE_BVH)) return RB_OK;
    const auto t_begin = Clock::now();
    if (device_builder(e, RB_FLAG_SPHERE_TREE_HOST, RB_FLAG_SPHERE_TREE_DEVICE, n >= kSphereDeviceBuildMin)) {
        HIP_TRY(e, t.nodes.resize(sphere_tree_node_capacity(n)));
        HIP_TRY(e, t.leaf.resize(n * 4));
        HIP_TRY(e, t.id.resize(n));
        DeviceSphereTreeInfo info{};
        const int rc = device_sphere_bvh_build(e->spheres.ptr, static_cast<uint32_t>(n), t.nodes.ptr, t.leaf.ptr, t.id.ptr, &info, e->stream);
        if (rc) return fail(e, RB_ERR_DEVICE, "device sphere tree build failed: %s", hipGetErrorString(static_cast<hipError_t>(rc)));
        if (sphere_stack_entries(info.depth) > kStackDepth) return RB_OK;   // beyond 16 M spheres: the scan (the host's tree is as deep)
        t.root = info.root;
        t.depth = sphere_stack_entries(info.depth);
        t.rec = {"device-median", ms_since(t_begin)};
        return RB_OK;
    }
    std::vector<SphereNode4> nodes;
    std::vector<uint32_t> order;
    uint32_t levels4 = 0;
    sphere_bvh_build(s, n, nodes, order, &t.root, &levels4);
    if (sphere_stack_entries(levels4) > kStackDepth) return RB_OK;
    t.depth = sphere_stack_entries(levels4);
    std::vector<float> leaf(n * 4);   // {centre, radius} = the first 16 bytes of an rb_sphere (rb_abi.h)
    for (size_t j = 0; j < n; ++j) std::memcpy(&leaf[j * 4], &s[order[j]], 4 * sizeof(float));
    int rc = upload(e, t.nodes, nodes.data(), nodes.size(), true);
    if (!rc) rc = upload(e, t.leaf, leaf.data(), leaf.size(), true);
    if (!rc) rc = upload(e, t.id, order.data(), order.size(), true);
    if (rc) return rc;
    HIP_TRY(e, hipStreamSynchronize(e->stream));  // the vectors above are locals
    t.rec = {"host-median", ms_since(t_begin)};
    return RB_OK;
}

// RB_FLAG_BUILD_TREE: the canonical reference-layout tree of the n triangles just uploaded (host copy `src`, borrowed for the
// update), in place of the caller's bvh_nodes / bvh_indices.  On the device by default: the nodes are read back (48 B per 128
// triangles) for validation and the host walks' builders, the indices stay on the device (fetched back by ensure_host_mesh if a
// host builder needs them).  A device short of memory for the builder's scratch falls back to the host builder: the same tree.
int build_engine_tree(rb_engine* e, const rb_gpu_triangle* src, size_t n) {
    const auto t_begin = Clock::now();
    e->prep_dirty = true;
    e->tree = {};
    std::vector<rb_bvh_node> nodes;
    std::vector<uint32_t> idx;
    const char* builder = n ? "host" : "";   // n == 0 (Delete, or an empty vector): an empty tree
    if (n && device_builder(e, RB_FLAG_BUILD_TREE_HOST, 0u, true)) {
        const size_t nn = bvh_node_count(n);
        HIP_TRY(e, e->nodes.resize(nn));
        HIP_TRY(e, e->indices.resize(n));
        const int brc = device_reference_bvh_build(e->tris.ptr, static_cast<uint32_t>(n), e->nodes.ptr, e->indices.ptr, e->stream);
        if (brc != hipSuccess && brc != hipErrorOutOfMemory)
            return fail(e, RB_ERR_DEVICE, "device tree build failed: %s", hipGetErrorString(static_cast<hipError_t>(brc)));
        if (brc == hipErrorOutOfMemory) (void)hipGetLastError();   // short of scratch: the host builder makes the same tree
        if (brc == hipSuccess) {
            nodes.resize(nn);
            HIP_TRY(e, hipMemcpyAsync(nodes.data(), e->nodes.ptr, sizeof(rb_bvh_node) * nn, hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(e, hipStreamSynchronize(e->stream));
            builder = "device";
        }
    }
    const bool on_device = builder[0] == 'd';
    if (!on_device) {   // the host builder, or the empty tree
        if (n) bvh_build_canonical(src, n, nodes, idx);
        int rc = upload(e, e->nodes, nodes.data(), nodes.size(), true);
        if (!rc) rc = upload(e, e->indices, idx.data(), idx.size(), true);
        if (rc) return rc;
        if (n) HIP_TRY(e, hipStreamSynchronize(e->stream));   // `nodes` / `idx` are moved below, but the copies read them now
    }
    commit_own_tree(e->sc, std::move(nodes), n);
    if (n == 0 || mesh_walks(e->opt).host_mesh) {   // the device builder's indices stay on the device until a host builder asks
        e->host_index_len = n;
        e->host_indices_stale = on_device;
        e->host_indices = std::move(idx);
    }
    if (n) e->tree = {builder, ms_since(t_begin)};
    return RB_OK;
}

// The chunked walk's tree: the caller's tree with the library's own levels below its leaves.
int build_chunk_tree(rb_engine* e, uint32_t tri_count) {
    ChunkAccel& t = e->chunk;
    if (!mesh_walks(e->opt).chunk || !mesh_takes_tree(e, tri_count)) return RB_OK;
    const auto t_begin = Clock::now();
    const uint32_t n_tris = std::min<uint32_t>(tri_count, static_cast<uint32_t>(e->host_tri_len));
    const uint32_t n_idx = static_cast<uint32_t>(e->host_index_len), n_nodes = static_cast<uint32_t>(e->sc.host_nodes.size());
    const char* builder = "";
    size_t n = 0;
    if (chunk_tree_on_device(e, n_idx) && n_idx <= e->indices.count && n_tris <= e->tris.count) {
        DeviceChunkTree dt;
        const int brc = device_chunk_tree_build(e->tris.ptr, n_tris, e->indices.ptr, n_idx, e->sc.host_nodes.data(), n_nodes, kStackDepth, &dt, e->stream);
        if (brc > 0) return fail(e, RB_ERR_DEVICE, "chunk tree build failed: %s", hipGetErrorString(static_cast<hipError_t>(brc)));
        if (brc == 0) {   // (-1: not for this builder, the host's decides)
            t.nodes.adopt(dt.nodes, dt.nodes_capacity);
            t.rank_slot.adopt(dt.rank_slot, dt.n_pos);
            t.pos_slot.adopt(dt.pos_slot, dt.n_pos);
            t.pos_rank.adopt(dt.pos_rank, dt.n_pos);
            t.n_nodes = dt.n_nodes;
            t.root = dt.root;
            t.depth = dt.depth;
            n = dt.n_pos;
            builder = "device";
        }
    }
    if (!builder[0]) {
        ChunkTree ct;
        if (const int rc = ensure_host_mesh(e)) return rc;
        if (!chunk_tree_build(e->host_tris.data(), n_tris, e->host_indices.data(), n_idx, e->sc.host_nodes.data(), n_nodes, kStackDepth, ct))
            return RB_OK;   // another walk takes this mesh
        n = ct.pos_slot.size();
        int rc = upload(e, t.nodes, ct.nodes.data(), ct.nodes.size(), true);
        if (!rc) rc = upload(e, t.rank_slot, ct.rank_slot.data(), ct.rank_slot.size(), true);
        if (!rc) rc = upload(e, t.pos_slot, ct.pos_slot.data(), n, true);
        if (!rc) rc = upload(e, t.pos_rank, ct.pos_rank.data(), n, true);
        if (rc) return rc;
        HIP_TRY(e, hipStreamSynchronize(e->stream));  // `ct` is a local
        t.n_nodes = ct.nodes.size();
        t.root = ct.root;
        t.depth = ct.depth;
        builder = "host";
    }
    for (DevBuf<float>* abc : {&t.a, &t.b, &t.c}) HIP_TRY(e, abc->resize(n * 4));
    if (launch_chunk_gather(e->ptris.ptr, t.pos_slot.ptr, t.pos_rank.ptr, static_cast<uint32_t>(n), t.a.ptr, t.b.ptr, t.c.ptr, e->stream))
        return fail(e, RB_ERR_DEVICE, "chunk gather launch failed");
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    t.rec = {builder, ms_since(t_begin)};
    return RB_OK;
}

// The library's own tree over the same triangles: the device builder from kDeviceBuildMinTriangles
// up (milliseconds instead of ~0.15 s per million triangles), the host's binned SAH below.
int build_own_tree(rb_engine* e, uint32_t tri_count) {
    OwnAccel& t = e->own;
    if (!mesh_walks(e->opt).own(tri_count) || !mesh_takes_tree(e, tri_count)) return RB_OK;
    int rc = ensure_host_mesh(e);
    if (rc) return rc;
    FastTree ft;
    const auto t_begin = Clock::now();
    const uint32_t n_idx = static_cast<uint32_t>(e->host_indices.size()), n_nodes = static_cast<uint32_t>(e->sc.host_nodes.size());
    const uint32_t n_tris = std::min<uint32_t>(tri_count, static_cast<uint32_t>(e->host_tris.size()));
    const float small_cap = (e->opt.flags & RB_FLAG_SKIP_NEAR_DEGENERATE) ? 0.0f : kFastSmallCap;
    const char* builder = "";
    DeviceTreeInfo info{};
    if (device_builder(e, RB_FLAG_HOST_BVH, RB_FLAG_DEVICE_BVH, n_tris >= kDeviceBuildMinTriangles)) {
        // reference-order metadata on the host (one pass over the caller's tree), the tree on the device
        if (fast_bvh_prepare(e->host_tris.data(), n_tris, e->host_indices.data(), n_idx, e->sc.host_nodes.data(), n_nodes, ft, small_cap) &&
            ft.slots.size() >= 1024) {
            const uint32_t n = static_cast<uint32_t>(ft.slots.size());
            const bool lbvh = (e->opt.flags & RB_FLAG_DEVICE_LBVH) != 0u;
            DevBuf<uint32_t> visit_slots;
            rc = upload(e, visit_slots, ft.slots.data(), ft.slots.size(), true);
            if (!rc) rc = upload(e, t.slot_meta, ft.slot_meta.data(), ft.slot_meta.size(), true);
            if (rc) return rc;
            HIP_TRY(e, t.nodes.resize(n - 1));
            HIP_TRY(e, t.slots.resize(n));
            rc = device_fast_bvh_build(e->tris.ptr, e->indices.ptr, visit_slots.ptr, n, t.slot_meta.ptr, t.nodes.ptr, t.slots.ptr, &info,
                                       e->stream, lbvh);
            if (rc && rc != static_cast<int>(hipErrorNotReady))
                return fail(e, RB_ERR_DEVICE, "device BVH build failed: %s", hipGetErrorString(static_cast<hipError_t>(rc)));
            if (rc) info.depth = 0xFFFFFFFFu;  // clustering did not converge within its round limit: host builder
            // a tree deeper than the LDS stack spills to a global scratch column per lane, which only the
            // persistent kernels (bounded grid) get; otherwise use the depth-limited host builder
            bool usable = info.depth <= kStackDepth;
            if (!usable && kernel_of(e->opt) != RB_KERNEL_PIXEL && info.depth <= 128u) {
                const size_t lanes = stream_kernel_max_threads(e->opt._reserved[0]);
                HIP_TRY(e, t.stack_overflow.resize(lanes * (info.depth - kStackDepth)));
                usable = true;
            }
            if (usable) builder = lbvh ? "device-lbvh" : "device-ploc";
        }
    }
    if (!builder[0]) {
        if (!fast_bvh_build(e->host_tris.data(), n_tris, e->host_indices.data(), n_idx, e->sc.host_nodes.data(), n_nodes, kStackDepth, ft, small_cap))
            return RB_OK;  // keep the reference walk
        rc = upload(e, t.nodes, ft.nodes.data(), ft.nodes.size(), true);
        if (!rc) rc = upload(e, t.slots, ft.slots.data(), ft.slots.size(), true);
        if (rc) return rc;
        info = DeviceTreeInfo{ft.root, ft.depth, ft.margin, ft.root_amax, {ft.bmin[0], ft.bmin[1], ft.bmin[2]}, {ft.bmax[0], ft.bmax[1], ft.bmax[2]}};
        builder = "host-sah";
    }
    rc = upload(e, t.slot_meta, ft.slot_meta.data(), ft.slot_meta.size(), true);
    if (!rc) rc = upload(e, t.ref_parent, ft.ref_parent.data(), ft.ref_parent.size(), true);
    if (!rc) rc = upload(e, t.gnodes, ft.gnodes.data(), ft.gnodes.size(), true);
    if (!rc) rc = upload(e, t.gslots, ft.gslots.data(), ft.gslots.size(), true);
    if (rc) return rc;
    HIP_TRY(e, t.tris.resize(t.slots.count));
    if (launch_gather_tris(e->ptris.ptr, t.slots.ptr, static_cast<uint32_t>(t.slots.count), t.tris.ptr, e->stream))
        return fail(e, RB_ERR_DEVICE, "gather kernel launch failed");
    HIP_TRY(e, hipStreamSynchronize(e->stream));  // `ft` is a local
    t.info = info;
    t.rec = {builder, ms_since(t_begin)};
    return RB_OK;
}

uint32_t accel_params(const rb_engine* e, KParams& p) {
    // a single-node reference-layout tree is walked without a stack (rb_kernels.hip, intersect_bvh); the mesh walks' trees go
    // with the caller's tree they were built over
    const bool multi_node = p.u.bvh_node_count > 1u;
    const bool tree_current = multi_node && p.u.bvh_node_count == e->sc.n_nodes;
    const bool use_chunk = e->chunk.rec.built() && tree_current;
    // (the caller's tree's need counts too: with no_leaf_stepping the launch falls to the per-segment kernel, which walks it)
    return std::max({multi_node ? std::max(e->sc.bvh_stack, 1u) : 0u, params(e->chunk, use_chunk, p),
                     params(e->own, !use_chunk && e->own.rec.built() && tree_current, (e->opt.flags & RB_FLAG_SKIP_NEAR_DEGENERATE) != 0u, p),
                     params(e->sph, e->sph.rec.built() && p.u.spheres_count == e->sc.n_spheres, p)});
}

}  // namespace rb

// ============================================================== C ABI ======
extern "C" {

int rb_bvh_build(const rb_gpu_triangle* tris, size_t n_tris, rb_bvh_node* nodes_out, size_t nodes_capacity,
                 size_t* n_nodes, uint32_t* indices_out) {
    if (!n_nodes || (n_tris > 0 && !tris)) return RB_ERR_NULL_ARGUMENT;
    std::vector<rb_bvh_node> nodes;
    std::vector<uint32_t> indices;
    rb::bvh_build(tris, n_tris, nodes, indices);
    *n_nodes = nodes.size();
    if (!nodes_out) return RB_OK;
    if (nodes_capacity < nodes.size()) return RB_ERR_INVALID_BVH;
    std::memcpy(nodes_out, nodes.data(), nodes.size() * sizeof(rb_bvh_node));
    if (indices_out) std::memcpy(indices_out, indices.data(), indices.size() * sizeof(uint32_t));
    return RB_OK;
}

int rb_bvh_build_canonical(const rb_gpu_triangle* tris, size_t n_tris, rb_bvh_node* nodes_out, size_t nodes_capacity,
                           size_t* n_nodes, uint32_t* indices_out) {
    if (const int rc = rb::canonical_build_args(tris, n_tris, nodes_out, nodes_capacity, n_nodes)) return rc == rb::kSizeQuery ? RB_OK : rc;
    std::vector<rb_bvh_node> nodes;
    std::vector<uint32_t> indices;
    rb::bvh_build_canonical(tris, n_tris, nodes, indices);
    std::memcpy(nodes_out, nodes.data(), nodes.size() * sizeof(rb_bvh_node));
    if (indices_out) std::memcpy(indices_out, indices.data(), indices.size() * sizeof(uint32_t));
    return RB_OK;
}

int rb_bvh_build_device(int32_t device, const rb_gpu_triangle* tris, size_t n_tris, rb_bvh_node* nodes_out, size_t nodes_capacity,
                        size_t* n_nodes, uint32_t* indices_out) {
    if (const int rc = rb::canonical_build_args(tris, n_tris, nodes_out, nodes_capacity, n_nodes)) return rc == rb::kSizeQuery ? RB_OK : rc;
    if (n_tris == 0) return RB_OK;
    if (device >= 0 && hipSetDevice(device) != hipSuccess) return rb::fail(nullptr, RB_ERR_DEVICE, "hipSetDevice(%d) failed", device);
    rb::DevBuf<rb_gpu_triangle> d_tris;
    rb::DevBuf<rb_bvh_node> d_nodes;
    rb::DevBuf<uint32_t> d_idx;
    hipStream_t stream = nullptr;
    hipError_t st = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
    if (st == hipSuccess) st = d_tris.resize(n_tris);
    if (st == hipSuccess) st = d_nodes.resize(*n_nodes);
    if (st == hipSuccess) st = d_idx.resize(n_tris);
    if (st == hipSuccess) st = hipMemcpyAsync(d_tris.ptr, tris, sizeof(rb_gpu_triangle) * n_tris, hipMemcpyHostToDevice, stream);
    if (st == hipSuccess) st = static_cast<hipError_t>(rb::device_reference_bvh_build(d_tris.ptr, static_cast<uint32_t>(n_tris), d_nodes.ptr, d_idx.ptr, stream));
    if (st == hipSuccess) st = hipMemcpyAsync(nodes_out, d_nodes.ptr, sizeof(rb_bvh_node) * *n_nodes, hipMemcpyDeviceToHost, stream);
    if (st == hipSuccess && indices_out) st = hipMemcpyAsync(indices_out, d_idx.ptr, 4u * n_tris, hipMemcpyDeviceToHost, stream);
    if (st == hipSuccess) st = hipStreamSynchronize(stream);
    if (stream) (void)hipStreamSynchronize(stream);   // (the buffers are freed on return, after this)
    if (stream) (void)hipStreamDestroy(stream);
    if (st != hipSuccess) return rb::fail(nullptr, RB_ERR_DEVICE, "device tree build failed: %s", hipGetErrorString(st));
    return RB_OK;
}

int rb_engine_tree(rb_engine* e, rb_bvh_node* nodes_out, size_t nodes_capacity, size_t* n_nodes, uint32_t* indices_out,
                   size_t indices_capacity, size_t* n_indices) {
    if (!e || !n_nodes || !n_indices) return RB_ERR_NULL_ARGUMENT;
    rb_engine* g = e;
    std::unique_lock<std::mutex> group_lock;
    if (rb::is_group(e)) {   // the handle's own lock first, then the part's (every part holds the same tree)
        group_lock = std::unique_lock<std::mutex>(g->mu);
        e = e->parts[0].get();
    }
    std::lock_guard<std::mutex> lock(e->mu);
    const size_t nn = e->sc.host_nodes.size(), ni = nn ? e->sc.n_indices : 0;
    *n_nodes = nn;
    *n_indices = ni;
    if (nodes_out) {
        if (nodes_capacity < nn) return rb::fail(g, RB_ERR_INVALID_BVH, "nodes_out holds %zu of %zu nodes", nodes_capacity, nn);
        if (nn) std::memcpy(nodes_out, e->sc.host_nodes.data(), sizeof(rb_bvh_node) * nn);
    }
    if (indices_out && ni) {
        if (indices_capacity < ni) return rb::fail(g, RB_ERR_INVALID_BVH, "indices_out holds %zu of %zu indices", indices_capacity, ni);
        rb::set_device(e);
        HIP_TRY(e, hipStreamSynchronize(e->stream));
        HIP_TRY(e, hipMemcpy(indices_out, e->indices.ptr, 4u * ni, hipMemcpyDeviceToHost));
    }
    return RB_OK;
}

const char* rb_tree_builder(const rb_engine* e, float* build_ms) { return rb::report(e, build_ms, [](const rb_engine& p) { return p.tree; }); }
const char* rb_fast_bvh_builder(const rb_engine* e, float* build_ms) { return rb::report(e, build_ms, [](const rb_engine& p) { return p.own.rec; }); }
const char* rb_sphere_tree_builder(const rb_engine* e, float* build_ms) { return rb::report(e, build_ms, [](const rb_engine& p) { return p.sph.rec; }); }
const char* rb_chunk_tree_builder(const rb_engine* e, float* build_ms) { return rb::report(e, build_ms, [](const rb_engine& p) { return p.chunk.rec; }); }

// Test aid (host only): the chunked walk's tree for a mesh and a caller tree, with its invariants checked.
int rb_debug_chunk_tree(const rb_gpu_triangle* tris, size_t n_tris, const rb_bvh_node* nodes, size_t n_nodes, const uint32_t* indices,
                        size_t n_indices, uint64_t out6[6]) {
    if (!tris || !nodes || !indices || !out6) return RB_ERR_NULL_ARGUMENT;
    if (n_tris >= (1ull << 31) || n_nodes >= (1ull << 31) || n_indices >= (1ull << 31)) return RB_ERR_INVALID_BVH;
    std::string why;
    if (!rb::bvh_validate(nodes, static_cast<uint32_t>(n_nodes), rb::kStackDepth, why, nullptr)) return rb::fail(nullptr, RB_ERR_INVALID_BVH, "%s", why.c_str());
    rb::ChunkTree t;
    for (int i = 0; i < 6; ++i) out6[i] = 0;
    if (!rb::chunk_tree_build(tris, static_cast<uint32_t>(n_tris), indices, static_cast<uint32_t>(n_indices), nodes,
                              static_cast<uint32_t>(n_nodes), rb::kStackDepth, t))
        return RB_OK;   // out6[0] == 0: this tree is left to another walk
    return rb::check_and_count(nullptr, "chunk tree", t, tris, static_cast<uint32_t>(n_tris), indices, static_cast<uint32_t>(n_indices), out6);
}

int rb_debug_engine_chunk_tree(rb_engine* e, uint64_t out6[6]) {
    if (!e || !out6) return RB_ERR_NULL_ARGUMENT;
    if (rb::is_group(e)) e = e->parts[0].get();
    std::lock_guard<std::mutex> lock(e->mu);
    rb::set_device(e);
    for (int i = 0; i < 6; ++i) out6[i] = 0;
    const rb::ChunkAccel& c = e->chunk;
    if (!c.rec.built()) return RB_OK;
    rb::ChunkTree t;
    const size_t n = c.rank_slot.count;
    t.root = c.root;
    t.depth = c.depth;
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    HIP_TRY(e, rb::read_back(t.nodes, c.nodes.ptr, c.n_nodes));
    HIP_TRY(e, rb::read_back(t.pos_slot, c.pos_slot.ptr, n));
    HIP_TRY(e, rb::read_back(t.pos_rank, c.pos_rank.ptr, n));
    HIP_TRY(e, rb::read_back(t.rank_slot, c.rank_slot.ptr, n));
    if (const int rc = rb::ensure_host_mesh(e)) return rc;
    const uint32_t n_tris = std::min<uint32_t>(e->prep_tri_count, static_cast<uint32_t>(e->host_tris.size()));
    const std::string what = std::string("chunk tree (") + c.rec.builder + " builder)";
    return rb::check_and_count(e, what.c_str(), t, e->host_tris.data(), n_tris, e->host_indices.data(), static_cast<uint32_t>(e->host_indices.size()), out6);
}

// Test aids: the library's own triangle tree and the sphere tree, handed out unchecked (tests/_tree_model.py judges them).
int rb_debug_own_tree(const rb_gpu_triangle* tris, size_t n_tris, const rb_bvh_node* nodes, size_t n_nodes, const uint32_t* indices,
                      size_t n_indices, rb_debug_own_node* nodes_out, size_t nodes_capacity, uint32_t* slots_out, size_t slots_capacity,
                      uint32_t* slot_meta_out, size_t slot_meta_capacity, uint64_t counts3[3], uint32_t root_depth[2], float bounds6[6]) {
    if (!tris || !nodes || !indices || !counts3 || !root_depth || !bounds6) return RB_ERR_NULL_ARGUMENT;
    if (n_tris >= (1ull << 31) || n_nodes >= (1ull << 31) || n_indices >= (1ull << 31)) return RB_ERR_INVALID_BVH;
    std::string why;
    if (!rb::bvh_validate(nodes, static_cast<uint32_t>(n_nodes), rb::kStackDepth, why, nullptr)) return rb::fail(nullptr, RB_ERR_INVALID_BVH, "%s", why.c_str());
    rb::FastTree ft;
    const bool built = rb::fast_bvh_build(tris, static_cast<uint32_t>(n_tris), indices, static_cast<uint32_t>(n_indices), nodes,
                                          static_cast<uint32_t>(n_nodes), rb::kStackDepth, ft);
    rb::OwnTreeCopy c;
    if (built) c = {ft.nodes.size(), ft.slots.size(), ft.slot_meta.size(), ft.root, ft.depth, ft.bmin, ft.bmax};
    if (const int rc = rb::own_tree_header(nullptr, c, nodes_out, nodes_capacity, slots_out, slots_capacity, slot_meta_out, slot_meta_capacity,
                                           counts3, root_depth, bounds6))
        return rc;
    if (nodes_out && c.n_nodes) std::memcpy(nodes_out, ft.nodes.data(), sizeof(rb::SphereNode) * c.n_nodes);
    if (slots_out && c.n_slots) std::memcpy(slots_out, ft.slots.data(), 4u * c.n_slots);
    if (slot_meta_out && c.n_meta) std::memcpy(slot_meta_out, ft.slot_meta.data(), 4u * c.n_meta);
    return RB_OK;
}

int rb_debug_engine_own_tree(rb_engine* e, rb_debug_own_node* nodes_out, size_t nodes_capacity, uint32_t* slots_out, size_t slots_capacity,
                             uint32_t* slot_meta_out, size_t slot_meta_capacity, uint64_t counts3[3], uint32_t root_depth[2], float bounds6[6]) {
    if (!e || !counts3 || !root_depth || !bounds6) return RB_ERR_NULL_ARGUMENT;
    if (rb::is_group(e)) e = e->parts[0].get();
    std::lock_guard<std::mutex> lock(e->mu);
    rb::set_device(e);
    const rb::OwnAccel& o = e->own;
    rb::OwnTreeCopy c;
    if (o.rec.built()) c = {o.nodes.count, o.slots.count, o.slot_meta.count, o.info.root, o.info.depth, o.info.bmin, o.info.bmax};
    if (const int rc = rb::own_tree_header(e, c, nodes_out, nodes_capacity, slots_out, slots_capacity, slot_meta_out, slot_meta_capacity,
                                           counts3, root_depth, bounds6))
        return rc;
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    if (nodes_out && c.n_nodes) HIP_TRY(e, hipMemcpy(nodes_out, o.nodes.ptr, sizeof(rb::SphereNode) * c.n_nodes, hipMemcpyDeviceToHost));
    if (slots_out && c.n_slots) HIP_TRY(e, hipMemcpy(slots_out, o.slots.ptr, 4u * c.n_slots, hipMemcpyDeviceToHost));
    if (slot_meta_out && c.n_meta) HIP_TRY(e, hipMemcpy(slot_meta_out, o.slot_meta.ptr, 4u * c.n_meta, hipMemcpyDeviceToHost));
    return RB_OK;
}

int rb_debug_sphere_tree(const rb_sphere* spheres, size_t n, rb_debug_sphere_node* nodes_out, size_t nodes_capacity, float* leaf_out,
                         uint32_t* id_out, size_t spheres_capacity, uint64_t counts2[2], uint32_t root_depth[2]) {
    if (!spheres || !counts2 || !root_depth) return RB_ERR_NULL_ARGUMENT;
    if (n == 0 || n >= (1u << 27)) return rb::fail(nullptr, RB_ERR_INVALID_BVH, "a sphere tree takes 1 to 2^27 - 1 spheres");
    std::vector<rb::SphereNode4> nodes;
    std::vector<uint32_t> order;
    uint32_t root = 0, levels4 = 0;
    rb::sphere_bvh_build(spheres, n, nodes, order, &root, &levels4);
    if (const int rc = rb::sphere_tree_header(nullptr, nodes.size(), n, root, rb::sphere_stack_entries(levels4), nodes_out, nodes_capacity,
                                              leaf_out, id_out, spheres_capacity, counts2, root_depth))
        return rc;
    if (nodes_out && !nodes.empty()) std::memcpy(nodes_out, nodes.data(), sizeof(rb::SphereNode4) * nodes.size());
    if (id_out) std::memcpy(id_out, order.data(), 4u * n);
    if (leaf_out)   // {centre, radius} = the first 16 bytes of an rb_sphere, as build_sphere_bvh uploads them
        for (size_t j = 0; j < n; ++j) std::memcpy(&leaf_out[j * 4], &spheres[order[j]], 4 * sizeof(float));
    return RB_OK;
}

int rb_debug_engine_sphere_tree(rb_engine* e, rb_debug_sphere_node* nodes_out, size_t nodes_capacity, float* leaf_out, uint32_t* id_out,
                                size_t spheres_capacity, uint64_t counts2[2], uint32_t root_depth[2]) {
    if (!e || !counts2 || !root_depth) return RB_ERR_NULL_ARGUMENT;
    if (rb::is_group(e)) e = e->parts[0].get();
    std::lock_guard<std::mutex> lock(e->mu);
    rb::set_device(e);
    const rb::SphereAccel& s = e->sph;
    const bool built = s.rec.built();
    const size_t nn = built ? s.nodes.count : 0, n = built ? s.id.count : 0;
    if (const int rc = rb::sphere_tree_header(e, nn, n, built ? s.root : 0u, built ? s.depth : 0u, nodes_out, nodes_capacity, leaf_out, id_out,
                                              spheres_capacity, counts2, root_depth))
        return rc;
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    if (nodes_out && nn) HIP_TRY(e, hipMemcpy(nodes_out, s.nodes.ptr, sizeof(rb::SphereNode4) * nn, hipMemcpyDeviceToHost));
    if (leaf_out && n) HIP_TRY(e, hipMemcpy(leaf_out, s.leaf.ptr, 16u * n, hipMemcpyDeviceToHost));
    if (id_out && n) HIP_TRY(e, hipMemcpy(id_out, s.id.ptr, 4u * n, hipMemcpyDeviceToHost));
    return RB_OK;
}

}  // extern "C"
