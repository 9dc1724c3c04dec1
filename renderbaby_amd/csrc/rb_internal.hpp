// rb_internal.hpp -- declarations shared by the runtime (rb_runtime.cpp), the queries (rb_queries.cpp), the
// BVH helper (rb_bvh.cpp) and the kernels (rb_kernels.hip and the other .hip files).  Not part of the ABI.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/rb_abi.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define RB_HD __host__ __device__
#else
#define RB_HD
#endif

namespace rb {

constexpr uint32_t kStackDepth = 32;      // per-lane traversal stack entries (LDS)
// The traversal stacks of a block are ONE region of LDS, s_stack[entry][thread]: 4-byte entries in columns of
// KParams::stack_depth entries, sized by launch_render.  Every walk a kernel runs -- the caller's tree, the chunked or the
// library's tree, and the sphere tree inside segment_finish -- uses the calling lane's column, one walk at a time.  An entry
// wider than kStackEntryBytes, or a walk deeper than stack_depth, runs into the neighbouring lane's column (r03: an
// experiment with 8-byte entries in k_trace_chunk did, and a lane popped a corrupted reference: a GPU memory fault).  The
// kernels assert the entry size where they take their column (StackColumn), the runtime the depth where it sets
// stack_depth (stack_depth_covers).
constexpr uint32_t kStackEntryBytes = 4;
constexpr uint32_t kDefaultStripeRows = 8;   // = the kernel tile's 8 rows: a tile's rays stay neighbours, the shards stay balanced (profiles/r04_shard_rehearsal.txt)

// ---- rb_bvh.cpp
void bvh_build(const rb_gpu_triangle* tris, size_t n_tris, std::vector<rb_bvh_node>& nodes,
               std::vector<uint32_t>& indices);
bool bvh_validate(const rb_bvh_node* nodes, uint32_t node_count, uint32_t max_stack, std::string& why,
                  uint32_t* depth_out);
// The canonical reference-layout tree: bvh_build's topology with every choice it leaves open fixed --
// (centroid, index) order, leaves in ascending index, boxes under the total order -0 < +0.  The caller has refused non-finite
// vertices (first_non_finite).
void bvh_build_canonical(const rb_gpu_triangle* tris, size_t n_tris, std::vector<rb_bvh_node>& nodes,
                         std::vector<uint32_t>& indices);
// index of the first triangle with a non-finite vertex coordinate, or n_tris
size_t first_non_finite(const rb_gpu_triangle* tris, size_t n_tris);
// What follows from the triangle count alone (identical for bvh_build and the canonical builders): the nodes with their
// children and leaf ranges and zero boxes, and the nodes of each depth in order of their first triangle (= pre-order within a
// depth) with the triangle range of each.
struct TreeSkeleton {
    std::vector<rb_bvh_node> nodes;
    std::vector<uint32_t> level_nodes;   // node indices, depth by depth
    std::vector<uint32_t> level_first;   // per entry of level_nodes: the node's first triangle ...
    std::vector<uint32_t> level_count;   // ... and its triangle count
    std::vector<uint32_t> level_begin;   // depth d = level_nodes[level_begin[d] .. level_begin[d + 1])
};
void bvh_skeleton(size_t n_tris, TreeSkeleton& sk);
size_t bvh_node_count(size_t n_tris);   // = bvh_skeleton(n_tris).nodes.size(), without building it

// The two-box node of the library's own TRIANGLE tree (leaves of <= 2: 0x80000000 | (count-1) << 28 | first).
struct alignas(16) SphereNode {
    float lmin[3];
    uint32_t left;    // child reference: node index, or leaf = 0x80000000 | (count-1) << 28 | first
    float lmax[3];
    uint32_t right;
    float rmin[3];
    uint32_t _pad0;
    float rmax[3];
    uint32_t _pad1;
};
static_assert(sizeof(SphereNode) == 64, "SphereNode is 64 B");
// ---- Sphere acceleration structure (no reference counterpart: shader.wgsl:574-586 scans; BASELINE C4 has 10^6 spheres).
// A 4-wide tree: every node holds the boxes of up to four children (two levels of median splits collapsed into one), so a
// ray's walk makes half as many DEPENDENT node fetches as with two-box nodes -- the walk waits on them (r04: 48 % of wave
// cycles with two-box nodes).  128 B, component-major, so the four box tests read like one.  Leaves are runs of at most
// kSphLeaf spheres of the leaf order: consecutive 16-byte {centre, radius} records (sph_leaf) with their original indices
// beside them (sph_id), tested one sphere per lane by k_trace_sph.
#ifndef RB_SPH_LEAF
#define RB_SPH_LEAF 16
#endif
constexpr uint32_t kSphLeaf = RB_SPH_LEAF;   // spheres per leaf = lanes per (ray, leaf) pair of k_trace_sph: 8 or 16
static_assert(kSphLeaf == 8 || kSphLeaf == 16, "a sphere leaf is tested by 8 or 16 lanes");
constexpr uint32_t kSphNone = 0xFFFFFFFFu;
struct alignas(16) SphereNode4 {
    float cx[4], cy[4], cz[4], hx[4], hy[4], hz[4];   // child k's box: centre (cx[k], cy[k], cz[k]) -+ half extents (hx[k], hy[k], hz[k]), rounded outwards
    uint32_t ref[4];   // child reference: kSphNone | node index | leaf = 0x80000000 | (count-1) << 27 | first (count <= kSphLeaf)
    uint32_t axes;     // children 0,1 = the lower half of the split along axis (axes & 3), cut along (axes >> 2) & 3; children 2,3 = the
    uint32_t _pad[3];  // upper half, cut along (axes >> 4) & 3: a ray visits the halves, and the children of a half, in the order of its direction's signs
    // lo .. hi -> centre and half extents that contain it whatever the rounding (the slab test then costs 6 operations per axis instead of 8)
    RB_HD void set_box(int k, const float lo[3], const float hi[3]) {
        float* c[3] = {cx, cy, cz};
        float* h[3] = {hx, hy, hz};
        for (int a = 0; a < 3; ++a) {
            const float m = 0.5f * lo[a] + 0.5f * hi[a];
            const float d0 = m - lo[a], d1 = hi[a] - m, d = d0 > d1 ? d0 : d1;
            c[a][k] = m;
            h[a][k] = d >= 0.0f ? d * 1.0000004f + 1e-37f : 0.0f;   // (d rounded up: one ulp for the subtraction, one for this product)
        }
    }
};
static_assert(sizeof(SphereNode4) == 128, "SphereNode4 is 128 B");
constexpr uint32_t kSphereBvhThreshold = 64;  // use the linear two-pass scan up to this many spheres
constexpr uint32_t kSphereDeviceBuildMin = 1024;  // from here up the sphere tree is built on the device by default
// host builder (rb_bvh.cpp): median splits on the longest axis of the centres.  depth = 4-wide levels.
void sphere_bvh_build(const rb_sphere* spheres, size_t n, std::vector<SphereNode4>& nodes,
                      std::vector<uint32_t>& order, uint32_t* root_ref, uint32_t* depth);
// The same tree made on the device (rb_build.hip): level by level, every level one segmented sort of the centres along each
// segment's longest axis -- the median splits of the host builder, a complete tree.  `spheres` is the device copy; nodes_out
// holds sphere_tree_node_capacity(n) nodes, leaf_out n float4 {centre, radius}, id_out n original indices.  Synchronises `stream`.
struct DeviceSphereTreeInfo {
    uint32_t root, depth, n_nodes;
};
size_t sphere_tree_node_capacity(size_t n);
int device_sphere_bvh_build(const rb_sphere* spheres, uint32_t n, SphereNode4* nodes_out, float* leaf_out, uint32_t* id_out,
                            DeviceSphereTreeInfo* info_out, void* stream);
// a node leaves at most three children waiting, so 3 entries per level is all a walk can hold at once (not one more: for
// C4's eight levels the 24-entry columns plus k_trace_sph's 15 KiB of wave corners are 39.4 KiB per block, four blocks per
// CU; a 25th entry would make it three)
inline uint32_t sphere_stack_entries(uint32_t levels4) { return 3u * levels4; }

// Walk of multi-node meshes when the caller's flags do not say: the chunked walk (ChunkTree below),
// at every size.  Should its tree not be buildable (a tree deeper than the LDS stack, a leaf root), the library's own
// tree of section 4.1 takes over from this many triangles up -- where the reference walk's ~450 triangle fetches per
// segment go to HBM -- and the reference walk below.  RB_FLAG_FAST_BVH / RB_FLAG_REFERENCE_WALK / RB_FLAG_CHUNK_WALK choose explicitly.
constexpr uint32_t kOwnTreeDefaultMinTriangles = 393216;
constexpr uint32_t kDeviceBuildMinTriangles = 16384;  // from here up the library's tree is built on the device by default

// c0 of the library's triangle walk (rb_device_intersect.hpp, FastWalk): hits with
// |cos(ray, triangle normal)| >= c0 are covered by the culling margin of the library's tree (FA in each node's two
// pad words), the others by a second pass over the reference tree guided by per-node normal cones.
constexpr float kFastGrazeCos = 0.03f;
// A triangle whose determinant bound L^2 / 1e-6 (the reference rejects |a^| < 1e-6) is at most this is "small": the
// culling margin of the library's tree then covers ALL its accepted hits, near-degenerate ones included, and the
// second pass skips it.  16000 <=> L <= 0.126: a margin of at most 2.6e-2 of the distance to the box.  A tuning
// constant, not part of the proof (any value up to 1.5e5 is covered): larger = fewer triangles left to the second
// pass but wider margins in the first (with RB_FLAG_SKIP_NEAR_DEGENERATE there is no second pass to relieve and the
// runtime passes 0: every triangle keeps the class (A) margin).  Measured (profiles/r02_small_cap_sweep.txt, M segments/s at 1500 / 8000 /
// 16000 / 32000 / 64000 / 150000): C5 744 / 1603 / 1600 / 1608 / 1604 / 1601, reference lamp scene 669 / 750 / 1066 /
// 1065 / 1102 / 909, C3 448 / 450 / 460 / 244 / 181 / 216.
#ifndef RB_FAST_SMALL_CAP
#define RB_FAST_SMALL_CAP 16000.0f
#endif
constexpr float kFastSmallCap = RB_FAST_SMALL_CAP;
constexpr uint32_t kSlotLarge = 0x80000000u;   // slot_meta[2 * slot + 1]: bit 31 = "large" triangle, low bits = reference rank
// A node of the reference tree as that second pass reads it: the caller's box and links bit for bit (the pass
// repeats the reference's own slab test), plus the cone {axis cos(alpha), tan(alpha)} of the triangle normals below.
struct alignas(16) GrazeNode {
    float bmin[3];
    uint32_t left;
    float bmax[3];
    uint32_t right;
    float cone[4];
    uint32_t first, count;   // leaf: range in FastTree::gslots (the leaf's LARGE triangles only)
    float cap;               // largest L^2 / 1e-6 over the large triangles below (+inf beyond 1.5e5): bounds how far from the
                             // node's box a near-degenerate hit can be reported, so the pass can cull on the best t
    uint32_t is_leaf;
};
static_assert(sizeof(GrazeNode) == 64, "GrazeNode is 64 B");

struct TriBound {
    double n[3] = {0, 0, 0};   // unit normal (if has_normal)
    float f = 0.0f;            // F_k: bound of L^2 / |a^| over the hits the library's tree answers for
    bool large = false, has_normal = false;
};
TriBound tri_bound(const rb_gpu_triangle& t, float small_cap = kFastSmallCap);

// The library's own triangle tree (rb_bvh.cpp).  Same 64-B two-box node as the sphere tree.
struct FastTree {
    std::vector<SphereNode> nodes;
    std::vector<GrazeNode> gnodes;     // per REFERENCE node: its box, links and the cone of the normals below it
    std::vector<uint32_t> gslots;      // the large triangles' slots, leaf by leaf (GrazeNode::first / count)
    uint32_t n_large = 0;              // triangles the second pass answers for ("large", rb_bvh.cpp)
    std::vector<uint32_t> slots;       // leaf order -> slot in bvh_indices order
    std::vector<uint32_t> slot_meta;   // per slot: {reference leaf node, rank in the reference visit order}
    std::vector<uint32_t> ref_parent;  // reference tree: parent of each node (root: 0)
    uint32_t root = 0x80000000u, depth = 0;
    float margin = 0.0f;               // slab-rounding part of the box inflation
    float bmin[3] = {0, 0, 0}, bmax[3] = {0, 0, 0};  // mesh bounds (for S, the per-ray distance bound)
    float root_amax = 0.0f;
    float small_cap = kFastSmallCap;   // the "small triangle" threshold the per-triangle bounds were made with
};
bool fast_bvh_build(const rb_gpu_triangle* tris, uint32_t tri_count, const uint32_t* indices, uint32_t index_len,
                    const rb_bvh_node* ref_nodes, uint32_t node_count, uint32_t stack_limit, FastTree& out,
                    float small_cap = kFastSmallCap);
// The part of it that depends on the reference tree only: ref_parent, slot_meta, and `slots` = the
// valid slots in the reference's visit order (the items a builder then arranges into a tree).
bool fast_bvh_prepare(const rb_gpu_triangle* tris, uint32_t tri_count, const uint32_t* indices, uint32_t index_len,
                      const rb_bvh_node* ref_nodes, uint32_t node_count, FastTree& out, float small_cap = kFastSmallCap);

// ---- The chunked walk (k_trace_chunk): the caller's tree on top, walked with the reference's
// own slab arithmetic on the reference's boxes (so a leaf is reached exactly when shader.wgsl:309-389 reaches it),
// nearer child first, and below every reference leaf the library's own small tree down to chunks of at most
// kChunkTris triangles, which a wavefront then tests cooperatively (one triangle per lane, coalesced records).
// A subtree is skipped only when the ray misses its box inflated by the margin that bounds how far from its
// triangle the reference's f32 Moller-Trumbore can report a hit (rb_device_intersect.hpp, FastWalk::entry), or
// enters it beyond the best t.  One 96-B node decides both children:
struct alignas(16) ChunkNode {
    float lmin[3];
    uint32_t lref;   // child reference: kChunkNone | leaf = bit 31, (count - 1) << 26, first position | node index, bit 30 = that node's children carry reference boxes
    float lmax[3];
    uint32_t rref;
    float rmin[3];
    uint32_t lfac;   // two bf16, rounded up: high = largest L^2 / 1e-6 below the child (bounds EVERY accepted hit), low = largest
    float rmax[3];   //   (L^2 / N) / (0.95 c0) (bounds the hits with |cos(ray, normal)| >= c0); 0x7F80 = +inf = always enter
    uint32_t rfac;
    float lcone[4];  // {axis cos(alpha), tan(alpha)} of the normals below the child (GrazeNode::cone): which of the two applies
    float rcone[4];
};
static_assert(sizeof(ChunkNode) == 96, "ChunkNode is 96 B");
#ifndef RB_CHUNK_TRIS
#define RB_CHUNK_TRIS 16
#endif
constexpr uint32_t kChunkTris = RB_CHUNK_TRIS;   // triangles per chunk = lanes per (ray, chunk) unit: 8, 16 or 32
static_assert(kChunkTris == 8 || kChunkTris == 16 || kChunkTris == 32, "a chunk is tested by 8, 16 or 32 lanes");
constexpr uint32_t kChunkNone = 0xFFFFFFFFu;
constexpr uint32_t kChunkLeaf = 0x80000000u, kChunkExact = 0x40000000u;
struct ChunkTree {
    std::vector<ChunkNode> nodes;
    std::vector<uint32_t> pos_slot;    // chunk order -> slot in bvh_indices order
    std::vector<uint32_t> pos_rank;    // chunk order -> rank in the reference's visit order (ties in t go to the lower rank)
    std::vector<uint32_t> rank_slot;   // rank -> slot (the winner's record for shading)
    uint32_t root = kChunkNone, depth = 0;
};
bool chunk_tree_build(const rb_gpu_triangle* tris, uint32_t tri_count, const uint32_t* indices, uint32_t index_len,
                      const rb_bvh_node* ref_nodes, uint32_t node_count, uint32_t stack_limit, ChunkTree& out);
bool chunk_tree_check(const ChunkTree& t, const rb_gpu_triangle* tris, uint32_t tri_count, const uint32_t* indices, uint32_t index_len,
                      uint32_t stack_limit, std::string& why);   // the structural invariants k_trace_chunk relies on

// ---- rb_build.hip: the chunked walk's tree built on the device: one thread block per reference leaf for the library's own
// levels, the caller's internal nodes by the host's bottom-up pass.  Returns 0 (built: the device arrays are the caller's
// to hipFree), -1 (not for this builder: a leaf beyond kChunkDeviceLeafMax triangles, or a tree the chunked walk does not
// take at all -- the host builder decides), or a hipError_t.
constexpr uint32_t kChunkDeviceLeafMax = 256;       // bvh.rs:12 MAX_LEAF_SIZE = 128
constexpr uint32_t kChunkDeviceBuildMin = 16384;    // slots from which the device builder is the default (below, the host's is microseconds)
struct DeviceChunkTree {
    ChunkNode* nodes = nullptr;
    size_t n_nodes = 0, nodes_capacity = 0;
    uint32_t *pos_slot = nullptr, *pos_rank = nullptr, *rank_slot = nullptr;
    size_t n_pos = 0;
    uint32_t root = kChunkNone, depth = 0;
};
int device_chunk_tree_build(const rb_gpu_triangle* d_tris, uint32_t tri_count, const uint32_t* d_indices, uint32_t index_len,
                            const rb_bvh_node* ref_nodes, uint32_t node_count, uint32_t stack_limit, DeviceChunkTree* out, void* stream);

// ---- rb_build.hip: the same tree built on the device (RB_FLAG_DEVICE_BVH), Morton order + LBVH
struct DeviceTreeInfo {
    uint32_t root, depth;
    float margin, root_amax;
    float bmin[3], bmax[3];
};
int device_fast_bvh_build(const rb_gpu_triangle* tris, const uint32_t* indices, const uint32_t* slots, uint32_t n,
                          const uint32_t* slot_meta, SphereNode* nodes_out, uint32_t* fast_slots_out, DeviceTreeInfo* info_out,
                          void* stream, bool plain_lbvh);
// ---- rb_build.hip: the canonical reference-layout tree (bvh_build_canonical's bytes) built on the device from d_tris (n
// finite triangles, 1 <= n < 2^31).  d_nodes holds bvh_skeleton(n).nodes.size() nodes, d_indices n.  Synchronises `stream`;
// returns a hipError_t (hipErrorOutOfMemory when its scratch does not fit).
int device_reference_bvh_build(const rb_gpu_triangle* d_tris, uint32_t n, rb_bvh_node* d_nodes, uint32_t* d_indices, void* stream);

// ---- device-side counters (one block of u64 in device memory)
enum Counter : uint32_t {
    C_SEGMENTS = 0, C_PATHS, C_NODES, C_TRIS, C_SPHERES, C_LIGHTS, C_MESH_HITS, C_COUNT
};

// Triangle in bvh_indices order with the per-triangle invariants of
// shader.wgsl:249-250,351 hoisted out of the per-ray loop.  edge1/edge2/normal
// are computed on the device by the same f32 operations the shader performs per
// test, so every ray sees bit-identical values.
struct alignas(16) PrepTri {   // 64 B: one s_load_dwordx16 (uniform) or four 16-B vector loads
    float v0[3];
    uint32_t tri_id;    // index into bvh_triangles (for hash_to_color and the :336 guard)
    float e1[3];        // v1 - v0
    uint32_t mesh_index;
    float e2[3];        // v2 - v0
    uint32_t valid;     // 0 when a guard of shader.wgsl:331,336 would `continue`
    float n[3];         // normalize(cross(e1, e2))  (shader.wgsl:351)
    uint32_t _pad;
};
struct alignas(16) PrepTriShade {   // 16 B: uv lookup indices (shader.wgsl:357-359)
    uint32_t v0_index;
    uint32_t v1_index;
    uint32_t v2_index;
    uint32_t _pad;
};

// The per-launch invariants of the sample loop (shader.wgsl:690,702-708), worked out once on the host by
// launch_render (host_cam in rb_kernels.hip: the same single IEEE binary32 operations, in the shader's order) so
// that no kernel holds twenty registers for them: a path start reads them from the kernel arguments.
struct Cam {
    float pos[3], right[3], up[3], fwd[3];
    float fov, aspect, wm1, hm1;
    float inv_wm1, inv_hm1;  // RN(1 / wm1), RN(1 / hm1) when fast_wh
    uint32_t fast_wh;        // both denominators inside the ranges the exact-reciprocal division was checked for
    uint32_t _pad;
};

// Everything a render launch needs.  Passed by value (kernarg segment => scalar loads).
// the stream kernels' queue words: one per group of blocks that share an XCD, 64 bytes apart
constexpr uint32_t kQueueGroups = 8, kQueueStride = 16, kQueueWords = kQueueGroups * kQueueStride;
struct KParams {
    rb_uniforms u;  // counts already patched (gpu_wrapper.rs:475-495) and clamped to buffer lengths
    const rb_sphere* spheres;
    const rb_point_light* lights;
    const rb_mesh* meshes;
    const rb_bvh_node* nodes;
    const uint32_t* indices;
    const rb_gpu_triangle* tris;
    const PrepTri* ptris;          // index_len entries, bvh_indices order
    const PrepTriShade* pshade;    // index_len entries
    const float* uvs;
    const uint32_t* tex_data;
    const rb_texture_info* tex_info;
    const float* srgb_lut;         // 256 entries: powf(i/255, 2.2) computed on the host
    const SphereNode* fast_nodes;  // fast triangle tree (nullptr => the reference walk)
    const GrazeNode* gnodes;       // per reference node: box, links, normal cone (the walk's second pass)
    const uint32_t* gslots;        // slots of the large triangles, leaf by leaf
    uint32_t fast_skip_second_pass; // RB_FLAG_SKIP_NEAR_DEGENERATE
    const float* fast_tris;        // PrepTri records gathered into fast-leaf order (64 B each)
    const uint32_t* fast_slots;    // fast-leaf order -> slot
    const uint32_t* slot_meta;     // per slot {reference leaf node, reference rank}
    const uint32_t* ref_parent;    // reference tree parents
    uint32_t fast_root;
    float fast_margin;
    float fast_bmin[3];
    float fast_root_amax;
    float fast_bmax[3];
    uint32_t _pad_fast;
    const ChunkNode* chunk_nodes;  // the chunked walk's tree (nullptr => another walk)
    const float* chunk_a;          // float4 per chunk-order position: v0, rank (as bits)
    const float* chunk_b;          // float4: e1, -
    const float* chunk_c;          // float4: e2, -
    const uint32_t* chunk_rank_slot; // rank -> slot
    uint32_t chunk_root;           // root child reference (the root's own box is nodes[0]'s)
    uint32_t chunk_n;              // positions
    const SphereNode4* sph_nodes;  // sphere tree (nullptr => linear scan)
    const float* sph_leaf;         // float4 {centre, radius} in leaf order
    const uint32_t* sph_id;        // original sphere index per leaf-order slot
    uint32_t sph_root;             // root child reference
    uint32_t _pad_sph;
    const float* accum_in;         // local_rows_padded * width * 4: the accumulation this launch resumes ...
    float* accum_out;              // ... and the one it writes (the same buffer, or the other frame slot when a pass runs ahead)
    uint32_t* out_rgba;            // local_rows_padded * width, x mirrored
    unsigned long long* counters;  // C_COUNT
    uint32_t* queue;               // work-queue head (RB_KERNEL_QUEUE / RB_KERNEL_STREAM)
    float* colors;                 // RB_KERNEL_STREAM: per-path radiance as float4, [tile][sample][64 pixels]
    uint32_t n_lights;             // arrayLength(&point_lights): >= 1 unless deleted
    uint32_t n_meshes;
    uint32_t index_len;            // arrayLength(&bvh_indices)
    uint32_t n_uvs;
    uint32_t n_tex;
    uint32_t first_pass, n_passes, samples_per_pass;
    uint32_t shard_rank, shard_count, stripe_rows, local_rows;  // local_rows: rows owned (unpadded)
    uint32_t stack_depth;          // LDS traversal-stack entries per lane (0 for single-node trees)
    uint32_t blocks_per_cu;        // persistent grid density (0 = default)
    uint32_t queue_batch;          // items a wave reserves per global atomic (RB_KERNEL_STREAM)
    uint32_t queue_groups;         // 1, or 8: one queue word per group of blocks that share an XCD (blockIdx % 8), each with its own stripes of items (set by launch_render)
    uint32_t queue_region;         // items per stripe (a multiple of queue_batch); stripe k belongs to band k % queue_groups
    uint32_t no_leaf_stepping;     // RB_KERNEL_STREAM: 1 = per-segment traversal even for multi-node trees
    uint32_t lds_mode;             // LDS staging of small meshes: 0 = when it fits, 1 = never
    uint32_t magic_S, magic_tiles_x; // floor(2^32 / d) for the item decode of the stream kernels (set by launch_render)
    uint32_t* stack_overflow;      // fast walk: entries beyond kStackDepth, [entry][grid * block] (nullptr if never needed)
    Cam cam;                       // set by launch_render
    const float* sph_scan;         // float4 {centre, radius * radius} per sphere, caller's order: pass 1 of the lean sphere scan
    // what the runtime has established of the scene for the plain walk (make_params; 0 = not known; no kernel reads it: plan_launch
    // picks the kernel by it): no segment of this launch reads a triangle's u, v or a texel
    uint32_t no_uv;
    // the triangle sift of a single-node tree (rb_tri_filter.hpp; sift_triangles): 1 = the table below serves this launch's node
    uint32_t sift;
    const float* sift_groups;      // SiftGroup records, 64 B each, in slot order
    uint32_t sift_block_ends;      // byte b: the groups of the list's blocks 0..b of 32 slots
    float sift_lo[3], sift_hi[3];  // the origin region: a lane whose origin is outside takes every slot
    float sift_kp, sift_ks, sift_kt, sift_kd;   // Sp_max times ChunkMargins' KP, KS (plus pass 1's own rounding), KT, KD
    float sift_rmax;               // the largest |1 / d| component for which no product of pass 1's slab values can overflow
};

struct LaunchInfo {
    uint32_t grid, block;
    size_t lds_bytes;
    const char* kernel_name;
    uint32_t trace_form;   // launch_render, the plain walk: RB_TRACE_FORM_* bits of the instantiation that ran (rb_abi.h); else 0
};

// The walk of a query over this scene with these flags -- rb_cast_rays' rule, which launch_query, launch_occluded and
// launch_radiance all ask: the chunked walk where its tree exists and leaf stepping is on; else the reference walk over the
// caller's tree (the library's own tree has no query form, so fast_nodes is dropped), stepped if there is a tree to step
// through -- a multi-node mesh tree or the spheres' -- and the plain per-ray kernel if there is none.
enum QueryWalk : uint32_t { kWalkPlain, kWalkBvh, kWalkChunk };
inline QueryWalk query_walk(KParams& p) {
    if (p.u.bvh_node_count > 1u && !p.no_leaf_stepping && p.chunk_nodes != nullptr) return kWalkChunk;
    p.fast_nodes = nullptr;
    return (p.u.bvh_node_count > 1u || p.sph_nodes != nullptr) ? kWalkBvh : kWalkPlain;
}

// ---- rb_query.hip: closest-hit queries.  One launch answers one piece: `n` rays of a device buffer, or
// the pixel centres of a window of the frame in DISPLAYED coordinates (x mirrored like the RGBA8 frame).  `hits` / `surf` are
// device buffers in the ABI's layout (record i = ray i, or window pixel (row, column) = row * win_w + column).
struct QueryArgs {
    const rb_ray* rays;       // nullptr: the pixel source
    rb_hit* hits;
    rb_surface* surf;         // may be nullptr
    uint32_t n;               // ray source: rays in this piece
    uint32_t win_x, win_y, win_w, win_h;   // pixel source: window origin (displayed x, row) and size
    uint32_t win_global;      // pixel source: rows are image rows (else this shard's local rows)
};
#ifndef RB_QUERY_PIECE_LOG2
#define RB_QUERY_PIECE_LOG2 22
#endif
// rays per launch: the query scratch is 128 + 192 + 192 MiB whatever n is (a frame piece: whole 8-row bands, so max(2^22, 8 x width)
// records).  2^20 cost the lamp fixture 1.76 instead of 1.22 ms of kernel time: every piece ends in a tail, and the copy-out of
// the piece before has pushed the tree out of L2 (five times the render's L2 misses per frame; profiles/r06_query_rate.txt)
constexpr uint32_t kQueryPiece = 1u << RB_QUERY_PIECE_LOG2;
int launch_query(const KParams& p, const QueryArgs& q, void* stream, LaunchInfo* info);
// ---- any-hit occlusion queries: the ray source of a QueryArgs (`hits` / `surf` unused) plus one bound
// per ray and one result byte per ray.  `tmax` may be nullptr (every ray: 1e20f); `mask`: RB_MASK_* stages that may occlude.
struct OcclArgs {
    QueryArgs q;
    const float* tmax;
    uint8_t* out;
    uint32_t mask;
};
int launch_occluded(const KParams& p, const OcclArgs& a, void* stream, LaunchInfo* info);
// ---- rb_radiance.hip: path-traced radiance along given rays.  One launch answers one piece: `n` rays of a
// device buffer, `samples` samples each, n x samples <= RB_TRACE_PIECE_ITEMS (rounded up to whole blocks of 64 rays).
struct RadArgs {
    const rb_ray* rays;       // the piece's rays
    const uint32_t* seeds;    // the piece's ray ids, or nullptr: seed_base + index in the piece
    float* colors;            // scratch: float4 per (ray, sample), [block of 64 rays][sample][64]
    rb_radiance* out;         // the piece's sums
    uint32_t* queue;          // one work-queue word
    uint32_t n;               // rays in this piece
    uint32_t seed_base;       // index of the piece's first ray in the call
    uint32_t first_sample, samples;
    uint32_t batch, magic_S;  // set by launch_radiance: items per reservation, floor(2^32 / samples)
};
// `records`: a.rays holds one record per (ray, sample) item in item order, made by launch_camera_rays (the k_cam kernels)
int launch_radiance(const KParams& p, const RadArgs& a, void* stream, LaunchInfo* info, bool records = false);
// ---- rb_camera.hip: camera rays made on the device.  One launch of k_cam_rays writes the records of one
// piece, 32 B each: {origin, seed after the generator's draws}, {normalised direction or 0 0 0 for an invalid ray, 0}.
struct CamGenArgs {
    rb_camera_ex cam;
    rb_ray* recs;             // item order: record (block * samples + sample) * 64 + pixel-in-block; linear: record i
    uint32_t* seeds;          // linear order only: seed i beside record i, whose fourth word is then 0
    uint32_t first_pixel;     // item order: the piece's first pixel; linear: the call's
    uint32_t n;               // item order: pixels in this piece; linear: items in this piece
    uint32_t item_base;       // linear: index in the call of the piece's first item, (pixel - first_pixel) * samples + sample
    uint32_t first_sample, samples;
    uint32_t linear;
};
int launch_camera_rays(const CamGenArgs& g, void* stream);
// ---- rb_hemisphere.hip: hemisphere rays made on the device.  One launch of k_hemi_rays writes the
// records of one piece of whole surfels, in k_cam_rays' format; k_hemi_count turns a piece's any-hit bytes into counts.
struct HemiGenArgs {
    const rb_surfel* surfels; // the piece's surfels
    const uint32_t* ids;      // the piece's surfel ids, or nullptr: id_base + index in the piece
    rb_ray* recs;             // item order: record (block * samples + sample) * 64 + surfel-in-block; linear: index * samples + sample
    uint32_t* seeds;          // linear order only, may be nullptr: seed i beside record i, whose fourth word is then 0
    float* tmax;              // linear order only, may be nullptr: `radius` per item, the bounds k_occl* read
    float offset, radius;
    uint32_t n;               // surfels in this piece
    uint32_t id_base;         // index of the piece's first surfel in the call
    uint32_t first_sample, samples;
    uint32_t linear;
};
int launch_hemisphere_rays(const HemiGenArgs& g, void* stream);
int launch_hemisphere_count(const uint8_t* occl, uint32_t n, uint32_t samples, rb_openness* out, void* stream);
// ---- rb_direct.hip: direct light at surface points.  The scene's emitter table is a compaction of its
// candidates -- triangles, then spheres, then lights -- in two steps, so that the caller can size the table between them:
// launch_emitter_count leaves every candidate's flag and exclusive offset in `work` (emitter_work_bytes) and the number that
// qualify in *count, launch_emitter_scatter writes their records.  One launch of k_light_rays writes the shadow rays of one
// piece of whole surfels with their bounds and contributions; k_direct_fold sums a piece's contributions under its any-hit bytes.
struct EmitArgs {
    const rb_gpu_triangle* tris;
    const rb_mesh* meshes;
    const rb_sphere* spheres;
    const rb_point_light* lights;
    uint32_t n_tris, n_meshes, n_spheres, n_lights;   // the counts a render sees: patched, clamped to the buffers
    uint32_t color_hash;                              // uniforms.color_hash_enabled: a triangle hit then reports no emission
};
uint64_t emitter_candidates(const EmitArgs& s);
size_t emitter_work_bytes(uint32_t total);   // 0: the scan could not be sized
int launch_emitter_count(const EmitArgs& s, void* work, uint32_t* count, void* stream);
int launch_emitter_scatter(const EmitArgs& s, const void* work, rb_emitter* out, uint32_t capacity, void* stream);
struct LightGenArgs {
    const rb_surfel* surfels; // the piece's surfels
    const uint32_t* ids;      // the piece's surfel ids, or nullptr: id_base + index in the piece
    const rb_emitter* emitters;   // n_emit records (<= RB_MAX_EMITTERS)
    rb_ray* recs;            // item order: record (block * samples + sample) * 64 + surfel-in-block; linear: index * samples + sample
    float* tmax;              // one bound per item, beside the record
    float* contrib;           // float4 per item: the unoccluded contribution, 1 or 0 for a valid or an invalid item
    float offset, shorten;
    uint32_t n_emit;
    uint32_t n;               // surfels in this piece
    uint32_t id_base;         // index of the piece's first surfel in the call
    uint32_t first_sample, samples;
    uint32_t linear;
};
// `cdf`: the pick weighted by g.n_emit inclusive uint32 weights in device memory (k_light_rays_cdf)
// ... with `grid`: one such table per cell of it, row after row (k_light_rays_grid)
int launch_light_rays(const LightGenArgs& g, void* stream, const uint32_t* cdf = nullptr, const rb_probe_grid* grid = nullptr);
// the table by power of em[n] into cdf[n] over `work` (emitter_cdf_work_bytes; 0: the scan could not be sized); queued, no wait
size_t emitter_cdf_work_bytes(uint32_t n);
int launch_emitter_cdf(const rb_emitter* em, uint32_t n, void* work, uint32_t* cdf, void* stream);
// the tables per cell of em[n] over `grid` into tables[rows * n], over `work` (emitter_grid_work_bytes); queued, no wait
size_t emitter_grid_work_bytes(uint32_t n);
// ... with `tally` (rows * n records, device memory) and `prior`: the learned weight (k_grid_rows_seen)
int launch_emitter_grid(const rb_emitter* em, uint32_t n, const rb_probe_grid& grid, void* work, uint32_t* tables, void* stream,
                        const rb_grid_tally* tally = nullptr, float prior = 0.0f);
// the count of one piece of a grid call behind its walk, added into tally[rows * g.n_emit] (k_grid_tally)
int launch_grid_tally(const LightGenArgs& g, const uint32_t* tables, const rb_probe_grid& cells, const uint8_t* occl, rb_grid_tally* tally,
                      void* stream);
int launch_direct_fold(const uint8_t* occl, const float* contrib, uint32_t n, uint32_t samples, uint32_t linear, rb_radiance* out, void* stream);
// ---- rb_probe.hip: irradiance probes made on the device.  One launch of k_probe_rays writes the records
// of one piece of whole probes, in k_cam_rays' format and k_hemi_rays' two orders; k_sh_project folds the colours launch_radiance
// left in RadArgs::colors with the SH9 basis of each record's direction.
struct ProbeGenArgs {
    const rb_probe* probes;   // the piece's probes
    const uint32_t* ids;      // the piece's probe ids, or nullptr: id_base + index in the piece
    rb_ray* recs;             // item order: record (block * samples + sample) * 64 + probe-in-block; linear: index * samples + sample
    uint32_t* seeds;          // linear order only, may be nullptr: seed i beside record i, whose fourth word is then 0
    uint32_t n;               // probes in this piece
    uint32_t id_base;         // index of the piece's first probe in the call
    uint32_t first_sample, samples;
    uint32_t linear;
};
enum : uint32_t { kProbeShapePlain = 1, kProbeShapeSplit = 2 };   // k_sh_project: one wave per 64 probes, or three with three coefficients each
constexpr uint32_t kProbeShapeDefault = kProbeShapePlain;
int launch_probe_rays(const ProbeGenArgs& g, void* stream);
int launch_sh_project(const float* colors, const rb_ray* recs, uint32_t n, uint32_t samples, rb_sh9* out, uint32_t shape, void* stream);
// ---- rb_probe_light.hip: light points from a baked probe grid.  k_probe_coeffs scales the sums of
// rb_bake_probes to coefficients, one lane per probe, in place if asked; k_probe_light blends the eight probes round each
// point, one lane per point.
struct ProbeLightArgs {
    rb_probe_grid grid;       // checked by the caller: counts >= 1, nx ny nz <= 2^31 - 64
    const rb_sh9* coeffs;     // nx ny nz records, x fastest
    const rb_surfel* points;
    rb_lit* out;
    uint32_t m;               // points in this launch
};
int launch_probe_coeffs(const rb_sh9* sums, uint32_t n, rb_sh9* out, void* stream);
enum : uint32_t { kLightShapePairs = 1, kLightShapeWide = 2 };   // k_probe_light: two corners' loads in flight, or all eight
constexpr uint32_t kLightShapeDefault = kLightShapePairs;
int launch_probe_light(const ProbeLightArgs& a, uint32_t shape, void* stream, const char** kernel_name = nullptr);
// ---- rb_probe_depth.hip, rb_probe_visibility.hip: probe visibility.  k_depth_project folds the hits of
// a piece's records -- launch_probe_rays in LINEAR order, launch_query over them -- into each probe's octahedral map, one wave
// per probe; k_probe_moments divides the sums, one wave per probe, in place if asked; k_probe_light_vis is k_probe_light with
// every corner's weight times the wrapped cosine and the Chebyshev bound of the corner's map.
enum : uint32_t { kDepthShapeLds = 1, kDepthShapeReadlane = 2 };   // k_depth_project's fold: the row parked in LDS, or lane j's words read across
constexpr uint32_t kDepthShapeDefault = kDepthShapeLds;   // 0.081 against 0.143 ms per 2^22 items
// out[i] = the sums of probe i < n; `shape`: kDepthShape* or 0 = the default, or RB_DEPTH_SHAPE in the environment
int launch_depth_project(const rb_ray* recs, const rb_hit* hits, uint32_t n, uint32_t samples, float max_distance, rb_probe_depth* out,
                         uint32_t shape, void* stream);
int launch_probe_moments(const rb_probe_depth* sums, uint32_t n, rb_probe_depth* out, float* share, void* stream);   // share may be nullptr
int launch_probe_light_vis(const ProbeLightArgs& a, const rb_probe_depth* moments, const rb_light_visibility& prm, void* stream);
// ---- rb_lightmap.hip: lightmap texels made on the device.  The triangles are PrepTri / PrepTriShade
// records in TRIANGLE order (launch_prep_tris over the identity order, launch_lightmap_iota), so that an owner is an index into
// bvh_triangles whatever bvh_indices hold.
struct LmArgs {
    const PrepTri* ptris;        // n_tris records, record t = triangle t
    const PrepTriShade* pshade;
    const float* uvs;
    uint32_t n_tris, n_uvs;
    uint32_t width, height, mesh, flags;
};
constexpr uint32_t kLmTile = 8;                    // a cover unit is one (triangle, 8 x 8-texel tile of the atlas inside its box)
constexpr uint64_t kLmPieceUnits = 1ull << 20;     // units per cover launch: 2^18 blocks of four waves, whatever the total
int launch_lightmap_iota(uint32_t* out, uint32_t n, void* stream);   // out[i] = i
size_t lightmap_work_bytes(uint32_t n_tris);       // the scratch lightmap_surfels needs at `work` (256-byte aligned)
// owners[width * height] and surfels[width * height] of the atlas, queued on `stream`; waits once, for the unit total that sizes
// the cover launches of at most `piece_units` units (0: kLmPieceUnits).  Returns a hipError_t.
int lightmap_surfels(const LmArgs& g, rb_surfel* surfels, uint32_t* owners, void* work, uint64_t piece_units, void* stream);
// sums[width * height] -> rgba: pass 0 and `dilate` passes that ping-pong between `out` and `tmp` (width * height float4 each;
// tmp may be nullptr when dilate is 0) and end in `out`
int launch_lightmap_resolve(const rb_radiance* sums, uint32_t width, uint32_t height, uint32_t dilate, float* out, float* tmp, void* stream);
Cam host_cam(const rb_uniforms& u);   // rb_kernels.hip: the camera of a launch, shader.wgsl:690,702-708

// ---- rb_denoise.hip: the edge-avoiding a-trous filter.  Everything is in the orientation of the delivered
// frame.  What a tap reads lies in three planes of 16-byte quads -- colour | class, normal | t, position | class of the guide --
// and the albedo, read by the prepare and finish steps only, in a fourth.
struct GuidePlanes {
    float* nt;    // float4 per pixel: normal, t
    float* pc;    // float4: pos, cls (as bits; the guide's class, before the prepare step's non-finite rule)
    float* al;    // float4: albedo, 0
};
enum : uint32_t { kDenoisePlain = 1, kDenoiseLds = 2 };   // the iteration kernel of steps 1 and 2: taps through L1 / L2, or a tile with its halo staged in LDS
struct DenoiseArgs {
    uint32_t w, h;
    const float* accum;     // the f32 accumulation (vec4 per pixel, shader x order: mirrored here), or nullptr ...
    const float* color4;    // ... then the mean radiance itself, vec4 per pixel
    GuidePlanes g;
    float* r[2];            // the two colour | class buffers the iterations ping-pong between, w * h float4 each
    float* linear_out;      // either may be nullptr
    uint32_t* rgba_out;
    uint32_t variant;       // 0 = the default (kDenoiseDefaultVariant), or RB_DENOISE_VARIANT in the environment (measurements)
};
bool denoise_params_valid(const rb_denoise_params& p, const char** why);
// prepare, the iterations, finish: asynchronous on `stream`; returns a hipError_t
int launch_denoise(const rb_denoise_params& prm, const DenoiseArgs& a, void* stream);
// first-hit records of the w x h pixel centres (displayed orientation) -> the guide planes; u: the scene's uniforms (the camera)
int launch_guide_pack(const rb_uniforms& u, const rb_hit* hits, const rb_surface* surf, uint32_t w, uint32_t h, const GuidePlanes& g, void* stream);
int launch_guide_split(const rb_guide* guides, size_t n, const GuidePlanes& g, void* stream);   // ABI records -> planes
int launch_guide_join(const GuidePlanes& g, size_t n, rb_guide* guides, void* stream);          // and back

// ---- rb_reproject.hip: temporal reprojection.  Frame records are float4 {mean r, g, b, count} per pixel;
// the guides are rb_denoise.hip's planes.
struct ReprojectArgs {
    uint32_t w, h;
    rb_view view;           // the previous camera
    const float* prev4;     // the previous frame's records ...
    GuidePlanes prev;       // ... and guides (read only)
    GuidePlanes cur;        // the current guides (read only)
    const float* cur4;      // nullptr: REPROJECT alone; else MERGE onto these records
    float* out4;
};
bool reproject_params_valid(const rb_reproject_params& p, const char** why);
bool view_finite(const rb_view& v);
// k_reproject, asynchronous on `stream`; returns a hipError_t
int launch_reproject(const rb_reproject_params& prm, const ReprojectArgs& a, void* stream);
// k_history_merge: out4 = MERGE(base, {mean radiance of the accumulation (shader x order: mirrored here), acc.w}) by g's classes
int launch_history_merge(uint32_t w, uint32_t h, const float* accum, const float* base, const GuidePlanes& g, float* out4, void* stream);

// ---- rb_kernels.hip
// All return hipError_t as int (0 = success); launches are asynchronous on `stream`.
// launch_render: k_pixel and k_queue whole; of the stream kernels the trace launch alone.  Its colours are summed by
// launch_accumulate (same KParams), on `stream` or on any stream that is ordered behind the trace launch.
int launch_render(const KParams& p, uint32_t kernel, bool stats, void* stream, LaunchInfo* info);
int launch_accumulate(const KParams& p, void* stream);
int launch_prep_tris(const rb_gpu_triangle* tris, uint32_t tri_count, const uint32_t* indices,
                     uint32_t index_len, PrepTri* out, PrepTriShade* shade, void* stream);
int launch_prep_materials(void* first_material, uint32_t stride, uint32_t n, void* stream);
int launch_prep_sphere_scan(const rb_sphere* spheres, uint32_t n, float* out, void* stream);   // float4 {centre, radius^2} per sphere
int launch_gather_tris(const PrepTri* ptris, const uint32_t* slots, uint32_t n, PrepTri* out, void* stream);
// prepared triangles -> the chunked walk's three float4 arrays in chunk order (A: v0 | rank, B: e1, C: e2)
int launch_chunk_gather(const PrepTri* ptris, const uint32_t* pos_slot, const uint32_t* pos_rank, uint32_t n, float* a,
                        float* b, float* c, void* stream);
// Multi-GPU assembly on the root device: gathered[rank][local row][x] (every rank's padded stripe buffer back to
// back) -> frame[global row][x]
int launch_deinterleave(const uint32_t* gathered, uint32_t* frame, uint32_t width, uint32_t height, uint32_t padded_rows,
                        uint32_t stripe_rows, uint32_t shard_count, void* stream);
size_t max_dynamic_lds(int device);   // hipDeviceAttributeMaxSharedMemoryPerBlock
int debug_tri_filter(const KParams& p, const float* rays, uint32_t n, uint32_t first, uint32_t end, uint32_t* out);   // rb_debug.hip: pass 1 of the sift, four mask words per ray; an RB_* status
int debug_walk_profile(unsigned long long* out64, int reset);   // pass occupancy counters of a profiling build, tools/ablate/rb_profile.patch (-1 otherwise)
int device_cu_count(int device);
uint32_t device_cu_count_cached();   // of the current device; asked once per device
uint32_t stream_kernel_max_threads(uint32_t blocks_per_cu);  // upper bound of grid * block of the stream kernels
// (the test hooks and measurement kernels -- rb_debug_*, rb_measure_* -- are whole in rb_debug.hip: kernel, launch and entry point)

}  // namespace rb
