/*
 * rb_abi.h -- C ABI of librenderbaby_hip.so, the MI355X (gfx950) backend for
 * RenderBaby's path-tracing hot path.
 *
 * This is the drop-in boundary: the entry points below are what a Rust shim
 * crate (`engine-hip`) binds with `extern "C"` to implement
 * `engine_config::Renderer` and `frame_buffer::FrameIterator`.  All citations
 * are file:line under the reference checkout (crates/... , src/...).
 *
 * Plain C: pointers, sizes, PODs.  No torch, no C++ types.  Inputs are borrowed
 * for the duration of a call only (copied to the device before return); the
 * library owns every device allocation; outputs go to caller-owned buffers.
 */
#ifndef RB_ABI_H
#define RB_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------ */
/* POD layouts -- byte-identical to the reference's #[repr(C)] GPU ABI types */
/* ------------------------------------------------------------------------ */

/* crates/engine-config/src/camera.rs:27-61 (48 B) */
typedef struct rb_camera {
    float pane_distance;
    float pane_width;
    float _pad0[2];
    float pos[3];
    float _pad1;
    float dir[3];
    float _pad2;
} rb_camera;

/* crates/engine-config/src/uniforms.rs:26-67 (144 B) */
typedef struct rb_uniforms {
    uint32_t width;
    uint32_t height;
    uint32_t total_samples;
    uint32_t color_hash_enabled;
    rb_camera camera;
    uint32_t spheres_count;
    uint32_t triangles_count;
    uint32_t bvh_node_count;
    uint32_t bvh_triangle_count;
    uint32_t bvh_root;
    float ground_height;
    uint32_t ground_enabled;
    uint32_t checkerboard_enabled;
    float sky_color[3];
    uint32_t max_depth;
    float checkerboard_color_1[3];
    uint32_t _pad1;
    float checkerboard_color_2[3];
    uint32_t _pad2;
} rb_uniforms;

/* crates/engine-config/src/material.rs:34-65 (80 B) */
typedef struct rb_material {
    float ambient[3];
    float _pad0;
    float diffuse[3];
    float _pad1;
    float specular[3];
    float shininess;
    float emissive[3];
    float ior;
    float opacity;
    uint32_t illum;
    int32_t texture_index;
    uint32_t _pad2;
} rb_material;

/* crates/engine-config/src/sphere.rs:34-43 (96 B) */
typedef struct rb_sphere {
    float center[3];
    float radius;
    rb_material material;
} rb_sphere;

/* crates/engine-config/src/point_lights.rs:23-33 (96 B) */
typedef struct rb_point_light {
    float center[3];
    float radius;
    rb_material material;
} rb_point_light;

/* crates/engine-config/src/mesh.rs:21-32 (96 B) */
typedef struct rb_mesh {
    uint32_t triangle_index_start;
    uint32_t triangle_count;
    uint32_t _pad[2];
    rb_material material;
} rb_mesh;

/* crates/engine-bvh/src/bvh.rs:18-34 (48 B) */
typedef struct rb_bvh_node {
    float aabb_min[3];
    uint32_t _pad0;
    float aabb_max[3];
    uint32_t _pad1;
    uint32_t left;
    uint32_t right;
    uint32_t first_primitive;
    uint32_t primitive_count;
} rb_bvh_node;

/* crates/engine-bvh/src/triangle.rs:9-29 (64 B) */
typedef struct rb_gpu_triangle {
    float v0[3];
    uint32_t v0_index;
    float v1[3];
    uint32_t v1_index;
    float v2[3];
    uint32_t v2_index;
    uint32_t mesh_index;
    uint32_t _pad0;
    uint32_t _pad1;
    uint32_t _pad2;
} rb_gpu_triangle;

/* crates/engine-config/src/texture.rs:26-36 -- Vec<u32> becomes ptr + w*h */
typedef struct rb_texture {
    uint32_t width;
    uint32_t height;
    const uint32_t* rgba_data; /* width*height texels, R in the low byte */
} rb_texture;

/* crates/engine-wgpu-wrapper/src/buffers.rs:13-25 (16 B); offset is in texels
 * (buffers.rs:151-168) */
typedef struct rb_texture_info {
    uint32_t offset;
    uint32_t width;
    uint32_t height;
    uint32_t _pad;
} rb_texture_info;

/* crates/engine-wgpu-wrapper/src/gpu_wrapper.rs:19-31 (16 B) */
typedef struct rb_progressive {
    uint32_t total_passes;
    uint32_t current_pass;
    uint32_t total_samples;
    uint32_t samples_per_pass;
} rb_progressive;

/* ------------------------------------------------------------------------ */
/* RenderConfig = 9 x Change<T>  (crates/engine-config/src/render_config.rs:37-57,99-109) */
/* ------------------------------------------------------------------------ */

enum {
    RB_KEEP = 0,   /* Change::Keep   */
    RB_CREATE = 1, /* Change::Create */
    RB_UPDATE = 2, /* Change::Update */
    RB_DELETE = 3  /* Change::Delete */
};

typedef struct rb_field {
    uint32_t change;  /* RB_KEEP.. */
    const void* ptr;  /* element array (may be NULL when count == 0) */
    size_t count;     /* number of ELEMENTS (uvs: number of f32) */
} rb_field;

typedef struct rb_config {
    rb_field uniforms;      /* 1 x rb_uniforms */
    rb_field spheres;       /* rb_sphere[] */
    rb_field uvs;           /* float[] (pairs) */
    rb_field meshes;        /* rb_mesh[] */
    rb_field lights;        /* rb_point_light[] */
    rb_field bvh_nodes;     /* rb_bvh_node[] */
    rb_field bvh_indices;   /* uint32_t[] */
    rb_field bvh_triangles; /* rb_gpu_triangle[] */
    rb_field textures;      /* rb_texture[] */
} rb_config;

/* ------------------------------------------------------------------------ */
/* Status codes.  1..10 mirror RenderConfigBuilderError
 * (crates/engine-config/src/render_config.rs:608-619); the rest replace the
 * reference's panics / anyhow errors.                                        */
/* ------------------------------------------------------------------------ */
enum {
    RB_OK = 0,
    RB_ERR_PANE_DISTANCE_OUT_OF_BOUNDS = 1,
    RB_ERR_PANE_WIDTH_OUT_OF_BOUNDS = 2,
    RB_ERR_INVALID_CAMERA_DIRECTION = 3,
    RB_ERR_INVALID_UNIFORMS = 4,
    RB_ERR_INVALID_SPHERES = 5,
    RB_ERR_INVALID_UVS = 6,
    RB_ERR_INVALID_MESHES = 7,
    RB_ERR_INVALID_LIGHTS = 8,
    RB_ERR_INVALID_TEXTURES = 9,
    RB_ERR_CANNOT_DELETE_NONEXISTENT = 10,
    RB_ERR_UNIFORMS_NOT_INITIALIZED = 11, /* gpu_wrapper.rs:313,321 panic */
    RB_ERR_NO_MORE_FRAMES = 12,           /* engine-pathtracer/src/lib.rs:170-177 */
    RB_ERR_INVALID_BVH = 13,              /* malformed tree (cycle, range, depth) */
    RB_ERR_UNSUPPORTED_DELETE = 14,       /* render_config.rs `todo!()` arms */
    RB_ERR_NULL_ARGUMENT = 15,
    RB_ERR_DEVICE = 16,                   /* HIP runtime failure */
    RB_ERR_NOT_INITIALIZED = 17,          /* render before the first update */
    RB_ERR_INVALID_OPTIONS = 18
};

typedef struct rb_engine rb_engine;

/* Options that have no counterpart in the reference (one wgpu device, whole
 * frame): device choice, row-stripe sharding for multi-GPU, launch shape. */
typedef struct rb_options {
    int32_t device;             /* HIP device ordinal; -1 = current */
    uint32_t shard_rank;        /* this engine renders stripes s with s % shard_count == shard_rank */
    uint32_t shard_count;       /* 0 or 1 = whole frame */
    uint32_t stripe_rows;       /* rows per stripe; 0 = default (8: the height of a kernel tile) */
    uint32_t passes_per_launch; /* samples per pixel folded into one kernel launch; 0 = default */
    uint32_t kernel;            /* RB_KERNEL_* ; 0 = default */
    uint32_t flags;             /* RB_FLAG_* */
    uint32_t _reserved[5];      /* tuning / ablation knobs, 0 = default: [0] persistent blocks per CU, [1] colour-buffer
                                   budget in MiB (default 4096, at most half of the free device memory), [2] items a wave
                                   reserves per queue atomic (a multiple of 64; multiples of 256 let the default kernel combine
                                   its colour stores), [3] 1 = no leaf stepping, [4] LDS staging of small meshes (1 = never) */
} rb_options;

enum {
    RB_KERNEL_DEFAULT = 0,
    RB_KERNEL_PIXEL = 1,  /* one thread per pixel, nested sample/depth loops */
    RB_KERNEL_QUEUE = 2,  /* persistent wavefronts, pixel queue + path regeneration */
    RB_KERNEL_STREAM = 3  /* persistent wavefronts over (pixel, sample) items + ordered accumulate pass */
};

enum {
    RB_FLAG_STATS = 1u, /* count nodes/tris/spheres/lights per segment (slower) */
    RB_FLAG_NO_SPHERE_BVH = 2u, /* always use the reference's linear sphere scan (shader.wgsl:574-586) */
    RB_FLAG_SPHERE_TREE_HOST = 2048u,   /* more than 64 spheres: build the library's sphere tree on the host (median splits) ... */
    RB_FLAG_SPHERE_TREE_DEVICE = 4096u, /* ... or on the device (the same splits, a segmented sort per level) whatever the count; by default the device
                                           builds it from 1024 spheres up.  The frame does not depend on the builder. */
    RB_FLAG_FAST_BVH = 4u, /* multi-node meshes: walk the library's own tree over the triangles (culling, near-first) plus
                              a second pass over the caller's tree for hits reported from near-zero determinants, and accept
                              a hit only if the reference's traversal would have tested it: argued and fuzzed to deliver the
                              reference walk's frames.  Without a walk flag the library uses the
                              chunked walk (RB_FLAG_CHUNK_WALK) */
    RB_FLAG_DEVICE_BVH = 8u, /* with RB_FLAG_FAST_BVH: build that tree on the GPU (Morton order + locally-ordered
                                clustering) instead of on the host (binned SAH): milliseconds instead of ~0.5 s per
                                million triangles, the same frames */
    RB_FLAG_DEVICE_LBVH = 16u, /* with RB_FLAG_DEVICE_BVH: plain LBVH instead of the clustering (ablation: faster
                                 build, slower walk) */
    RB_FLAG_REFERENCE_WALK = 32u, /* multi-node meshes: walk the caller's tree exactly as shader.wgsl:282-392 does
                                     (128-triangle leaves, fixed order, no culling); same frames, 2-5x slower */
    RB_FLAG_HOST_BVH = 64u, /* build the library's tree on the host (binned SAH) whatever the triangle count */
    RB_FLAG_GATHER_PEER_COPY = 128u, /* rb_create_multi: move the stripes with hipMemcpyPeerAsync instead of RCCL
                                        (hosts without librccl; several shards on one device in the tests) */
    RB_FLAG_NO_RUN_AHEAD = 256u, /* progressive iterator: do not start the next pass while a frame is read back */
    RB_FLAG_CHUNK_WALK = 1024u, /* multi-node meshes: the chunked walk, THE DEFAULT -- the caller's tree walked with the
                                   reference's own slab arithmetic (nearer child first, subtrees culled on the best t by the
                                   margin that bounds the reference's reported hits), the library's own levels below its
                                   leaves down to 16-triangle chunks, which a wavefront tests cooperatively, one triangle
                                   per lane.  Same frames: every hit goes through the reference's own
                                   triangle test, and the two rounding-error inequalities the culling rests on are derived
                                   mechanically (tools/margin_certify.py) and fuzzed against the oracle, not proven in a proof
                                   assistant -- RB_FLAG_REFERENCE_WALK, or RB_REFERENCE_WALK=1 in the environment of a host that
                                   cannot be rebuilt, walks the reference's way.  The flag only makes the choice explicit */
    RB_FLAG_CHUNK_TREE_HOST = 8192u,    /* the chunked walk's tree: build it on the host (one thread per granted CPU) ... */
    RB_FLAG_CHUNK_TREE_DEVICE = 16384u, /* ... or on the device (one thread block per reference leaf) whatever the mesh's size; by default the
                                           device builds it from 16 384 triangle slots up.  A caller's tree with leaves of more than 256
                                           triangles is built on the host either way.  The frame does not depend on the builder. */
    RB_FLAG_BUILD_TREE = 32768u,      /* the engine builds the reference-layout tree itself from bvh_triangles -- the canonical tree of
                                         rb_bvh_build_canonical, on the device (rb_bvh_build_device) -- so that the caller sends
                                         triangles only.  bvh_nodes and bvh_indices must then be RB_KEEP in every config (else
                                         RB_ERR_INVALID_BVH); the tree follows the triangles field: Create / Update rebuild it, Delete
                                         empties it, Keep keeps it.  Non-finite vertices are RB_ERR_INVALID_BVH.  Every walk works
                                         unchanged; rb_engine_tree reads the tree back, rb_tree_builder names its builder */
    RB_FLAG_BUILD_TREE_HOST = 65536u, /* the same, built on the host (rb_bvh_build_canonical: the same bytes).  Both flags together
                                         are RB_ERR_INVALID_OPTIONS */
    RB_FLAG_SKIP_NEAR_DEGENERATE = 512u /* with the library's tree: skip its second pass.  The walk then answers only for
                                           hits whose ray is more than ~1.7 degrees off the plane of a LARGE triangle
                                           (L^2 > 1.6e-2); a hit the reference reports from a near-zero determinant there can be
                                           missed.  Several times faster on coarse meshes; frames validated equal on the
                                           BASELINE scenes, but this is the one mode the exactness argument does not cover. */
};

/* Work counters, summed over every launch since the last rb_reset_stats.
 * `segments` is the throughput unit (one executed iteration of the bounce
 * loop, shader.wgsl:534); the rest feed the algorithmic-bytes formula of
 * SURVEY.md section 8(d) and are only filled when RB_FLAG_STATS is set. */
typedef struct rb_stats {
    uint64_t segments;
    uint64_t paths;
    uint64_t nodes_popped;
    uint64_t tris_tested;
    uint64_t spheres_tested;
    uint64_t lights_tested;
    uint64_t mesh_hits;
    uint64_t launches;
    double kernel_ms; /* sum of HIP-event durations of the render launch groups */
    double trace_ms;  /* of which: the trace / render kernels alone (k_trace*, k_queue, k_pixel) */
    double accumulate_ms; /* of which: k_accumulate (RB_KERNEL_STREAM only) */
} rb_stats;

/* ------------------------------------------------------------------------ */
/* Entry points                                                             */
/* ------------------------------------------------------------------------ */

/* Engine::new(rc) -- crates/engine-pathtracer/src/lib.rs:111-119 ->
 * GpuWrapper::new, gpu_wrapper.rs:82-105.  Requires Create for uniforms,
 * spheres, uvs, meshes, lights, textures (buffers.rs:74-97 panics otherwise;
 * here: NULL + rb_last_error(NULL)).  The engine is not yet "initialized":
 * the first rb_update must again carry Create (gpu_wrapper.rs:117-121). */
rb_engine* rb_create(const rb_config* cfg);
rb_engine* rb_create_ex(const rb_config* cfg, const rb_options* opt);

/* The same engine over several devices of this process (the reference has one wgpu
 * device, gpu_device.rs:27-70): the frame's rows are sharded in interleaved stripes (stripe s -> devices[s % n]),
 * every device renders all samples of its rows with global pixel indices, and each delivered frame is ONE RCCL
 * gather of the RGBA8 stripes to devices[0] (grouped ncclSend / ncclRecv over a communicator made with
 * ncclCommInitAll), de-interleaved there and read back -- so rb_render / rb_iter_next return the whole frame,
 * bit-identical to a single-device engine's.  opt->shard_* must be zero; every other entry point works on the
 * handle as on a single-device engine (statistics add up over the devices). */
rb_engine* rb_create_multi(const rb_config* cfg, const rb_options* opt, const int32_t* devices, uint32_t n_devices);

/* One process per device instead: every process creates its shard (rb_create_ex with shard_rank / shard_count),
 * rank 0 makes an id, the host program hands it to the others (any transport: MPI, a file, torch.distributed)
 * and all call rb_comm_init_rank.  From then on rb_render / rb_iter_next gather the stripes to rank 0, which
 * receives the whole frame; on the other ranks rgba_out may be NULL and nothing is written. */
#define RB_COMM_ID_BYTES 128
/* Can this process load RCCL at all (RB_OK) -- so that every rank can say so BEFORE the collective rb_comm_init_rank, and
 * one that cannot does not leave the others waiting inside it.  Loads the library and resolves its symbols, nothing else:
 * no id is made (ncclGetUniqueId opens a listening socket and starts a thread that waits for the ranks to check in). */
int rb_comm_available(void);
/* On rank 0 only. */
int rb_comm_unique_id(uint8_t id_out[RB_COMM_ID_BYTES]);
int rb_comm_init_rank(rb_engine* e, const uint8_t id[RB_COMM_ID_BYTES], uint32_t rank, uint32_t nranks);

/* What the exchange of a sharded engine looks like from inside: the communicator's size and this handle's rank AS RCCL
 * REPORTS THEM (ncclCommCount / ncclCommUserRank; 0 ranks when nothing goes through RCCL: a whole-frame engine, or the
 * peer-copy transport), and the duration of this rank's share of the last gather (root: receives + de-interleave, on
 * its exchange stream, HIP events).  Any pointer may be NULL.  No reference counterpart (one wgpu device). */
int rb_comm_info(rb_engine* e, uint32_t* rccl_ranks, uint32_t* rccl_rank, float* last_gather_ms);

/* drop(Engine) */
void rb_destroy(rb_engine* e);

/* GpuWrapper::update + update_uniforms -- gpu_wrapper.rs:116-300,469-576:
 * Change state machine, validate_init / validate
 * (render_config.rs:163-268), count patch-up, uploads. */
int rb_update(rb_engine* e, const rb_config* cfg);

/* GpuWrapper::dispatch_compute + read_pixels -- gpu_wrapper.rs:406-426,432-463:
 * zero accumulation, run all total_samples passes, return RGBA8 (w*h*4 bytes,
 * row-major, top row first, x mirrored, A=255) into rgba_out. */
int rb_render(rb_engine* e, uint8_t* rgba_out);

/* <Engine as Renderer>::render(rc) -- engine-pathtracer/src/lib.rs:58-71:
 * rb_update + rb_render in one call. */
int rb_render_config(rb_engine* e, const rb_config* cfg, uint8_t* rgba_out);

/* <Engine as Renderer>::frame_iterator(rc) -- lib.rs:86-96: rb_update, then
 * current_pass = 0.  One iterator per engine at a time (the reference shares
 * one GpuWrapper behind a mutex the same way). */
int rb_iter_begin(rb_engine* e, const rb_config* cfg);
/* RaytracerFrameIterator::has_next -- lib.rs:153-156 */
int rb_iter_has_next(rb_engine* e);
/* RaytracerFrameIterator::next -- lib.rs:169-228: first call zeroes the
 * accumulation; one pass; read back; current_pass += 1.
 * Exhausted => RB_ERR_NO_MORE_FRAMES ("No more frames available"). */
int rb_iter_next(rb_engine* e, uint8_t* rgba_out);
/* RaytracerFrameIterator::destroy -- lib.rs:231-233 */
void rb_iter_destroy(rb_engine* e);
/* Extension (per-N-pass delivery): every rb_iter_next advances `n` passes
 * (the last one whatever is left) in one launch chunk and reads back once, so a frame is delivered
 * every n samples instead of after each one -- the frames are the reference's frames n-1, 2n-1, ...
 * and the last.  n = 0 or 1 is the reference's behaviour (the default; restored by rb_create only).
 * Applies from the next rb_iter_next. */
int rb_iter_set_passes_per_frame(rb_engine* e, uint32_t n);

/* anyhow error text of the last failing call on `e` (or of rb_create when
 * e == NULL): a copy owned by the calling thread, valid until that thread's next rb_last_error. */
const char* rb_last_error(const rb_engine* e);

/* GpuWrapper::get_width/get_height -- gpu_wrapper.rs:317-329 */
int rb_get_size(const rb_engine* e, uint32_t* width, uint32_t* height);

/* ---- Lower-level control used by bench.py, the parity tests and the
 * multi-GPU gather.  No reference counterpart: the reference can only run
 * whole renders synchronously. ---- */

/* Zero the accumulation buffer (gpu_wrapper.rs:407-411). */
int rb_clear(rb_engine* e);
/* Launch passes [first_pass, first_pass+n_passes) asynchronously on the
 * engine's stream (dispatch_compute_progressive, gpu_wrapper.rs:365-400,
 * without the per-pass host sync). */
int rb_dispatch(rb_engine* e, uint32_t first_pass, uint32_t n_passes);
/* Optional: everything a dispatch of n_passes passes would set up lazily -- the prepared triangles and the library's own
 * levels of the tree (as rb_dispatch(e, 0, 0) does), and the stream kernels' colour buffer (up to 4 GiB of device memory) --
 * without tracing anything.  A host that times its first frame calls this first and does not time hipMalloc. */
int rb_reserve(rb_engine* e, uint32_t n_passes);
/* Wait for the engine's stream. */
int rb_sync(rb_engine* e);
/* Copy this engine's RGBA8 rows (mirrored, local stripe order) to the host. */
int rb_read_rgba(rb_engine* e, uint8_t* rgba_out);
/* Copy the f32 accumulation (vec4 per pixel, shader x order, local stripe
 * order) to the host: local_rows*width*4 floats. */
int rb_read_accumulation(rb_engine* e, float* accum_out);
/* Page-locked host memory for frames (extension): rb_render / rb_iter_next / rb_read_rgba recognise a
 * page-locked rgba_out (from here, or registered by the caller with hipHostRegister) and copy into it by DMA on
 * a second stream, without the staging and host-side copy a pageable destination costs -- with the iterator's
 * run-ahead pass this is what lets frame delivery run at the compute rate.  Plain malloc'ed buffers keep
 * working (blocking copy).  Free with rb_host_free. */
void* rb_host_alloc(size_t bytes);
void rb_host_free(void* p);

/* Device pointer + byte size of the RGBA8 buffer of the committed frame (a single engine: its local stripe
 * buffer, valid until the next iterator step; a multi-device handle: the assembled frame on devices[0]). */
int rb_device_rgba(rb_engine* e, void** d_ptr, size_t* bytes);
/* Number of image rows this engine owns (== height when not sharded) and
 * the padded row count of the local buffer (equal on every rank). */
int rb_local_rows(const rb_engine* e, uint32_t* rows, uint32_t* padded_rows);
/* Global row index of local row `local_row`. */
int rb_global_row(const rb_engine* e, uint32_t local_row, uint32_t* global_row);

/* Row-stripe sharding geometry as pure functions (no engine, no device): stripe s
 * (rows [s*stripe_rows, (s+1)*stripe_rows)) belongs to rank s % shard_count; a
 * rank stores its stripes back to back.  owned_rows = image rows the rank
 * renders; padded_rows = rows of its local buffer, equal on every rank so that
 * one equal-size gather moves the frame. */
int rb_shard_layout(uint32_t height, uint32_t shard_rank, uint32_t shard_count, uint32_t stripe_rows,
                    uint32_t* owned_rows, uint32_t* padded_rows);
/* Global image row of a rank's local row (may be >= height in the padding). */
uint32_t rb_shard_global_row(uint32_t shard_rank, uint32_t shard_count, uint32_t stripe_rows,
                             uint32_t local_row);

/* Counters and times of every launch since the last rb_reset_stats.  While the progressive iterator is running they
 * INCLUDE the pass group it has started ahead of the delivered frame (and one it later drops because the scene
 * changed): the device counts what it traces. */
int rb_get_stats(rb_engine* e, rb_stats* out);
int rb_reset_stats(rb_engine* e);
/* Duration of the most recent rb_dispatch launch group, HIP events on the
 * engine's stream (ms).  Synchronises. */
int rb_last_dispatch_ms(rb_engine* e, float* ms);

/* BVH::new -- crates/engine-bvh/src/bvh.rs:87-150: median split on the longest
 * axis, leaves of <= 128 triangles, pre-order numbering.  Two-call protocol:
 * pass nodes_out == NULL to query sizes.  indices_out must hold n_tris u32.
 * The top levels are built on several threads (a subtree's node count follows from its triangle count, so every
 * index is known beforehand): 10^6 triangles in 12 ms on 16 cores where one takes 133 -- the tree the reference
 * rebuilds on the CPU for every render (scene_engine_adapter.rs:435-440). */
int rb_bvh_build(const rb_gpu_triangle* tris, size_t n_tris,
                 rb_bvh_node* nodes_out, size_t nodes_capacity, size_t* n_nodes,
                 uint32_t* indices_out);

/* The canonical reference-layout tree: rb_bvh_build's topology, numbering and node count (they follow from n_tris alone) with
 * every choice BVH::new leaves open fixed -- centroids ((v0 + v1) + v2) / 3 in f32, ordered by (centroid along the axis, triangle
 * index) with -0 == +0, the left child the first count / 2 of its node in that order, leaves listed in ascending index, boxes
 * the min / max of the vertices under the total order in which -0 < +0.  Where no centroid tie
 * straddles a median it is rb_bvh_build's tree with every leaf sorted.  A non-finite vertex coordinate is RB_ERR_INVALID_BVH
 * (rb_last_error(NULL) names the triangle).  Same two-call protocol as rb_bvh_build, but the size query (nodes_out == NULL)
 * answers from n_tris alone, without building (tris may be NULL there); built on the host's threads. */
int rb_bvh_build_canonical(const rb_gpu_triangle* tris, size_t n_tris,
                           rb_bvh_node* nodes_out, size_t nodes_capacity, size_t* n_nodes,
                           uint32_t* indices_out);
/* The same bytes built on `device` (-1 = current): host arrays in and out, the build itself on the GPU (presorted id lists per
 * axis, one stable partition per depth).  The size query (nodes_out == NULL) touches no device and may pass tris == NULL. */
int rb_bvh_build_device(int32_t device, const rb_gpu_triangle* tris, size_t n_tris,
                        rb_bvh_node* nodes_out, size_t nodes_capacity, size_t* n_nodes,
                        uint32_t* indices_out);
/* Two-call read-back of the reference-layout tree the engine walks -- the caller's, or its own under RB_FLAG_BUILD_TREE:
 * pass nodes_out == NULL and indices_out == NULL to query n_nodes / n_indices.  Either array may be NULL to skip it. */
int rb_engine_tree(rb_engine* e, rb_bvh_node* nodes_out, size_t nodes_capacity, size_t* n_nodes,
                   uint32_t* indices_out, size_t indices_capacity, size_t* n_indices);
/* Which builder produced the tree the engine walks: "device", "host" (RB_FLAG_BUILD_TREE / _HOST), "caller" (sent in the
 * config), or "" when there is none.  `build_ms`, if not NULL, receives the wall time of the engine's own build with its
 * read-back of the nodes (0 for the caller's tree). */
const char* rb_tree_builder(const rb_engine* e, float* build_ms);

/* Test aid (host only, no device): builds the chunked walk's tree for this mesh and this caller tree and checks the
 * structural invariants the kernel relies on (every valid slot in exactly one chunk, ranks consistent, references in range,
 * depth within the stack, per child slot an unbounded margin or a box and a bound that cover the triangles below).
 * out6 = {built (0: this tree is left to another walk), nodes, positions, depth, chunks, child slots with an unbounded
 * margin}; a violated invariant is RB_ERR_INVALID_BVH with rb_last_error(NULL) naming it. */
int rb_debug_chunk_tree(const rb_gpu_triangle* tris, size_t n_tris, const rb_bvh_node* nodes, size_t n_nodes, const uint32_t* indices,
                        size_t n_indices, uint64_t out6[6]);
/* The same check on the tree an engine is walking (after the first rb_dispatch / rb_render that follows an update): the
 * chunked walk's arrays are read back from the device -- whichever builder made them -- and checked against the engine's
 * copy of the mesh.  out6 as above (built = 0: the engine has no chunked tree). */
int rb_debug_engine_chunk_tree(rb_engine* e, uint64_t out6[6]);
/* Test aids: the library's own triangle tree (RB_FLAG_FAST_BVH / _DEVICE_BVH / _DEVICE_LBVH / _HOST_BVH)
 * and its sphere tree, handed out as they are so that a test can hold them to their invariants (tests/_tree_model.py); nothing
 * is checked here.  One node of the triangle tree decides both children: their boxes, their references (node index, or leaf =
 * 0x80000000 | (count - 1) << 28 | first position in `slots`, count 1 or 2) and per child FA, the largest F_k below it (+inf:
 * always enter). */
typedef struct rb_debug_own_node {
    float lmin[3];
    uint32_t left;
    float lmax[3];
    uint32_t right;
    float rmin[3];
    float left_fa;
    float rmax[3];
    float right_fa;
} rb_debug_own_node;
/* One 4-wide node of the sphere tree: child k's box is (cx[k], cy[k], cz[k]) -+ (hx[k], hy[k], hz[k]); ref[k] is 0xFFFFFFFF
 * (no child), a node index, or leaf = 0x80000000 | (count - 1) << 27 | first position in the leaf order (count <= 16).
 * Children 0, 1 are the lower half of the split along axis (axes & 3), cut along (axes >> 2) & 3; children 2, 3 the upper
 * half, cut along (axes >> 4) & 3. */
typedef struct rb_debug_sphere_node {
    float cx[4], cy[4], cz[4], hx[4], hy[4], hz[4];
    uint32_t ref[4];
    uint32_t axes;
    uint32_t _pad[3];
} rb_debug_sphere_node;
/* Host only, no device: the host builder's triangle tree (fast_bvh_build) for this mesh and this caller tree.  Two calls:
 * with every out array NULL, counts3 = {nodes, slots (valid slots, in leaf order), slot_meta words (2 per index slot)} --
 * all 0 when this tree is left to another walk; then with arrays of at least those sizes.  root_depth = {root reference,
 * depth: the stack entries the walk is given}, bounds6 = the mesh bounds {min xyz, max xyz}.  slot_meta[2 * slot] is the
 * caller's leaf of the slot (0xFFFFFFFF: not a valid slot), slot_meta[2 * slot + 1] its rank, bit 31 = "large" triangle. */
int rb_debug_own_tree(const rb_gpu_triangle* tris, size_t n_tris, const rb_bvh_node* nodes, size_t n_nodes, const uint32_t* indices,
                      size_t n_indices, rb_debug_own_node* nodes_out, size_t nodes_capacity, uint32_t* slots_out, size_t slots_capacity,
                      uint32_t* slot_meta_out, size_t slot_meta_capacity, uint64_t counts3[3], uint32_t root_depth[2], float bounds6[6]);
/* The same arrays of the tree an engine walks, read back from the device whichever builder made them (after the first
 * rb_dispatch / rb_render that follows an update; a group handle answers with its first part).  The device builders leave
 * the nodes they collapsed into two-triangle leaves unreferenced and unwritten.  counts3 = {0, 0, 0}: no such tree. */
int rb_debug_engine_own_tree(rb_engine* e, rb_debug_own_node* nodes_out, size_t nodes_capacity, uint32_t* slots_out, size_t slots_capacity,
                             uint32_t* slot_meta_out, size_t slot_meta_capacity, uint64_t counts3[3], uint32_t root_depth[2], float bounds6[6]);
/* Host only, no device: the host builder's sphere tree (sphere_bvh_build) over n spheres.  Two calls as above: counts2 =
 * {nodes, spheres}; leaf_out takes 4 floats per sphere ({centre, radius} in leaf order), id_out the original index of each;
 * root_depth = {root reference, depth: stack entries = 3 per level of nodes}. */
int rb_debug_sphere_tree(const rb_sphere* spheres, size_t n, rb_debug_sphere_node* nodes_out, size_t nodes_capacity, float* leaf_out,
                         uint32_t* id_out, size_t spheres_capacity, uint64_t counts2[2], uint32_t root_depth[2]);
/* The same arrays of the sphere tree an engine walks (more than 64 spheres), read back from the device.  counts2 = {0, 0}:
 * the engine scans its spheres. */
int rb_debug_engine_sphere_tree(rb_engine* e, rb_debug_sphere_node* nodes_out, size_t nodes_capacity, float* leaf_out, uint32_t* id_out,
                                size_t spheres_capacity, uint64_t counts2[2], uint32_t root_depth[2]);
/* Which builder produced the chunked walk's tree: "device", "host", or "" when the engine walks another way.  Valid after the
 * first rb_dispatch / rb_render that follows an update; `build_ms`, if not NULL, receives the wall time of that build with
 * its uploads and the gather of the chunks' triangle records. */
const char* rb_chunk_tree_builder(const rb_engine* e, float* build_ms);
/* Measurement aid for the roofline record (bench.py): the rate at which this device serves divergent 16-byte gathers --
 * every lane its own 128-byte line of a table of `table_bytes` (0 = 2 MiB, L2-resident) -- in lane accesses per second:
 * the ceiling of the L1 / texture-address path that a lane-per-ray tree walk runs into. */
int rb_measure_l1_gather(int32_t device, uint64_t table_bytes, double* accesses_per_s);
/* Test hook: evaluates the device's f32 /, sqrt, normalize, u32->f32, min/max and
 * dot on n input pairs (out8n: 8*n floats) so tests can check them against
 * IEEE-754 results computed on the host. */
int rb_debug_math(const float* a, const float* b, float* out8n, uint32_t n);
/* Measurement aid: the pass / phase occupancy counters of a library built from sources with tools/ablate/rb_profile.patch
 * applied (tools/walk_profile.sh: k_trace_sph's passes and the lanes, pairs, rounds and survivors in them; k_trace's lanes per
 * phase of its loop body), summed over every launch since the last reset.  The product build carries no counting code and
 * returns RB_ERR_DEVICE. */
int rb_debug_walk_profile(uint64_t out64[64], int reset);
/* Test hook: checks the kernels' fast exact reciprocal against the compiler's correctly rounded
 * 1/b for all 2^23 significands (both signs) at one biased exponent; out16[0] = mismatch count. */
int rb_debug_rcp_exhaustive(uint32_t biased_exponent, uint32_t* out16);
/* Test hook: the same sweep for the reciprocal of the single-node walk's triangle test with its guard (both of its ways):
 * all 2^23 significands and both signs at one biased exponent (0..255) against 1.0f / x, bit patterns compared, a NaN equal to
 * a NaN; out16[0] = mismatch count, out16[1..15] = some offending bit patterns. */
int rb_debug_rcp_det_exhaustive(uint32_t biased_exponent, uint32_t* out16);
/* Test hook: the hand-laid triangle trip of the single-node trace kernels against the compiler-laid form of the same test on
 * `n` seeded (ray, triangle, incoming hit) triples plus constructed edge cases (determinant at its guards, u, v, u + v and t at
 * their bounds, NaN and infinity in the ray, lanes off on entry).  out32[0] = number of triples whose {t, u, v, slot} differ
 * in any bit (must be 0), out32[1] = index of one such triple, out32[2..17] = its o, d, v0, edge1, edge2, incoming hit.t,
 * out32[18..21] / out32[22..25] = the two results. */
int rb_debug_triangle_trip(uint32_t n, uint32_t seed, uint32_t* out32);
/* Test hook: the same sweep for the trip of the flat kernels (rb_debug_trace_form), which carries {t, slot} only: those two
 * words against the compiler-laid form's, bit for bit.  out32 as above (the u, v words repeat the compiler-laid form's). */
int rb_debug_triangle_trip_flat(uint32_t n, uint32_t seed, uint32_t* out32);
/* Test hook: the same sweep for the trip of the triangle sift's second pass (RB_TRACE_FORM_SIFT), which takes the triangle's record
 * per lane; uv = 0: the form that carries {t, slot}, else the one with u, v.  out32 as above. */
int rb_debug_triangle_trip_vec(uint32_t n, uint32_t seed, uint32_t uv, uint32_t* out32);
/* Test hook: the first pass of the triangle sift on `n` (at most 2^22) rays of six floats {origin, direction}, with the table of
 * the engine's single node and the origin region of its current camera and spheres: out[4 i + b] = ray i's candidate bits of
 * block b of 32 slots (bit k: slot first + 32 b + k; 0 for a block the list does not have), list2 = {first, end} of the node's list.  Conservative: every slot whose
 * triangle the reference's test accepts for the ray has its bit set.  RB_ERR_INVALID_OPTIONS if this engine's scene does not
 * sift (more than one node, a list beyond 128 slots, fewer than 4 live triangles, nothing to reject, a scene that carries u, v --
 * only the flat kernels sift --, RB_TRI_FILTER=0). */
int rb_debug_tri_filter(rb_engine* e, const float* rays, uint32_t n, uint32_t* out, uint32_t* list2);
/* Test hook: the root box of the single-node walk on `n` (at most 2^24) rays of six floats {origin, direction} and the box
 * box6 = {bmin, bmax}: out[i] bit 0 = the walk's slab test on its own reciprocals, bit 1 = the rule by which the single-node
 * trace kernels go past that test says the answer is known to be true (origin strictly inside a finite box, no NaN in the
 * direction).  Bit 1 must never be set without bit 0. */
int rb_debug_root_box(const float* rays, uint32_t n, const float* box6, uint32_t* out);
/* Test hook: the normalize of the single-node trace kernels (its general form and the form for the rejection loop's unit
 * vectors) against v / sqrt(dot(v, v)) with the correctly rounded / and sqrt, bit patterns compared, a NaN equal to a NaN.
 * xyz = n + n_unit vectors of three floats: the first n go through the general form, the next n_unit through the unit-vector
 * form (they must be points the rejection loop can accept: coordinates on its grid, 0 < dot < 1); then the unit-vector form
 * runs on the first try of the loop from each of the seeds seed0 .. seed0 + n_seeds - 1 where that try is accepted.
 * out16[0..2] = vectors that differ in the three groups (must be 0), out16[3] = accepted tries, out16[4] = 1 + index of one
 * differing vector (0: none), out16[5..7] = it, out16[8..10] = the form's result, out16[11..13] = the quotient's. */
int rb_debug_normalize_sites(const float* xyz, uint32_t n, uint32_t n_unit, uint32_t seed0, uint32_t n_seeds, uint32_t* out16);
/* Measurement aid (tools/salu_mix.py): a loop of independent v_fma_f32 at 8 waves per SIMD on every CU with `scalar_per_16`
 * (0, 4, 8, 12 or 16) independent scalar adds among each 16 of them and, if `branch` is not 0, one never-taken
 * s_cbranch_execz per 16.  out3 = {shader clocks per vector instruction and SIMD, shader clock in GHz, milliseconds}. */
int rb_measure_salu_mix(int32_t device, uint32_t scalar_per_16, uint32_t branch, double* out3);
/* Test hook: checks the kernels' one-rounding `rnd(seed) * 2 - 1` (one fma) against the shader's three operations on all
 * 2^32 seeds; out16[0] = number of seeds whose value differs, out16[1..15] = some of them. */
int rb_debug_rnd_pm1_exhaustive(uint32_t* out16);
/* Test hook: the same for the fast exact division a/b over a block of significand pairs
 * (denominators [b_begin, +b_count) x numerators [a_begin, +a_count), biased exponents ea, eb);
 * out16[0] = mismatch count, then up to 7 (a, b) bit patterns. */
int rb_debug_div_exhaustive(uint32_t b_begin, uint32_t b_count, uint32_t ea, uint32_t eb, uint32_t a_begin,
                            uint32_t a_count, unsigned long long* out16);

/* Name of the render kernel the most recent rb_dispatch used ("k_trace", "k_trace_bvh",
 * "k_queue", "k_pixel"). */
const char* rb_last_kernel_name(const rb_engine* e);
/* Test hook: which instantiation of "k_trace" the most recent rb_dispatch of the stream kernel ran -- RB_TRACE_FORM_* bits;
 * 0 for every other kernel.  A scene whose mesh and sphere materials all have texture_index < 0 (and, with the ground on, its
 * lights too: an empty lights vector leaves one zero-filled light of index 0) runs the FLAT kernels, which carry no
 * barycentrics through the triangle loop and have no texel lookup.  Same frames, bit for bit.  RB_TRACE_UV=1 in the environment
 * when an engine is made keeps it on the kernels that carry u, v, whatever the scene (A/B measurements, tests). */
enum {
    RB_TRACE_FORM_FLAT = 1u,    /* k_trace_flat / k_trace_flat_direct */
    RB_TRACE_FORM_SIFT = 2u,    /* with FLAT and STAGED: k_trace_sift, the single node's triangle list sifted by a conservative box test
                                 * per group of triangles, the exact test on each lane's own survivors (same frames, bit for bit;
                                 * RB_TRI_FILTER=0 in the environment when an engine is made keeps it on k_trace_flat) */
    RB_TRACE_FORM_BIG = 4u,     /* the 8-wave instantiation (large launches) */
    RB_TRACE_FORM_STAGED = 8u,  /* a row's paths started in one pass (else every lane starts its own) */
    RB_TRACE_FORM_MULTI = 16u   /* the per-segment ablation of a multi-node tree or a sphere tree */
};
uint32_t rb_debug_trace_form(const rb_engine* e);

/* ---- Closest-hit queries (no reference counterpart).  A query answers, for one ray: what does
 * `closest_hit` hold at shader.wgsl:603, after the ground, BVH, sphere and point-light stages of one bounce-loop iteration?
 * Same category order, strict `<`, `t > 0.001`, 1e20 start, phantom light, kept counts and numerics contract as a render of
 * the uploaded scene.  A query draws no random number and touches neither the accumulation, the RGBA8 frame, the colour
 * buffer nor the work counters (rb_get_stats does not move); a pass the progressive iterator has started ahead stays valid. */
typedef struct rb_ray { float origin[3]; float _pad0; float dir[3]; float _pad1; } rb_ray;          /* 32 B */
enum { RB_HIT_NONE = 0, RB_HIT_GROUND = 1, RB_HIT_TRIANGLE = 2, RB_HIT_SPHERE = 3, RB_HIT_LIGHT = 4,
       RB_HIT_INVALID = 0xFFFFFFFFu };
typedef struct rb_hit {                                                                             /* 48 B */
    float t;            /* closest_hit.t; 1e20f for NONE / INVALID */
    uint32_t kind;      /* RB_HIT_* */
    uint32_t prim;      /* triangle: index into bvh_triangles; sphere / light: its index; else 0xFFFFFFFF */
    uint32_t mesh;      /* triangle: its mesh_index; else 0xFFFFFFFF */
    float u, v;         /* triangle: the barycentrics intersect_triangle returned for the winner; else 0 */
    uint32_t _pad[2];
    float normal[3];    /* closest_hit.normal as the shader sets it (no flip); 0 for NONE / INVALID */
    float _pad1;
} rb_hit;
typedef struct rb_surface {                                                                         /* 48 B */
    float albedo[3];    /* what :644-651 would multiply into the attenuation (specular if is_metal, else diffuse x texture); 0 for NONE / INVALID */
    uint32_t flags;     /* bit 0 is_metal, bit 1 use_texture */
    float emissive[3];  /* closest_hit.material.emissive; NONE: uniforms.sky_color; INVALID: 0 */
    int32_t texture_index;
    float uv[2];        /* closest_hit.uv as the shader leaves it */
    float _pad[2];
} rb_surface;
/* n rays from host memory (pageable, or page-locked as rb_render recognises it) against the uploaded scene; hits_out[n], and
 * surf_out[n] unless NULL.  The device normalises `dir` (v / sqrt((x x + y y) + z z)) and measures t along the normalised
 * direction: the walks' culling margins are derived for |d| = 1 +- 4 ulp.  A ray whose origin or normalised direction has a
 * non-finite or all-zero component set (a zero direction, or one so long that its squared length overflows) is RB_HIT_INVALID and is not walked.  Rays go through the device in
 * pieces of at most 2^22 rays (128 MiB of rays, 2 x 192 MiB of records: the scratch does not grow with n).  n > 2^31 - 64 is
 * RB_ERR_INVALID_OPTIONS; n == 0 is RB_OK.
 * The walk is the one a render of this scene with this engine's flags takes: the chunked walk for multi-node meshes by
 * default, the per-lane reference walk under RB_FLAG_REFERENCE_WALK and for trees of at most one node, the sphere tree for
 * more than 64 spheres.  RB_FLAG_FAST_BVH engines are answered by the per-lane reference walk over the caller's tree: the
 * library's own tree has no query form (it returns the same winner by construction). */
int rb_cast_rays(rb_engine* e, const rb_ray* rays, size_t n, rb_hit* hits_out, rb_surface* surf_out);
/* One ray per pixel through the pixel CENTRE (the primary ray of the render with both jitter offsets 0), in the
 * orientation of the delivered RGBA8 frame: row-major, top row first, x mirrored -- a pixel of the displayed image indexes its
 * record.  A sharded engine delivers its padded_rows local rows in local stripe order like rb_read_accumulation (rows of the
 * padding: RB_HIT_INVALID); a multi-device handle the whole frame, computed on devices[0]. */
int rb_render_hits(rb_engine* e, rb_hit* hits_out, rb_surface* surf_out);
/* rb_render_hits for one displayed pixel (px from the left, py from the top of the whole image, also on a sharded engine). */
int rb_pick(rb_engine* e, uint32_t px, uint32_t py, rb_hit* hit_out, rb_surface* surf_out);
/* Name of the kernel the most recent query used ("k_query", "k_query_bvh", "k_query_chunk"; "" before the first). */
const char* rb_last_query_kernel_name(const rb_engine* e);
/* Measurement aid for tools/query_rate.py, not part of the query interface (it may change or go): kernel time of the most
 * recent query, HIP events around its launches, summed over the pieces, ms. */
int rb_last_query_ms(rb_engine* e, float* ms);

/* ---- Any-hit occlusion queries and device-resident ray buffers (no reference counterpart).  One bit per
 * ray: is anything between here and there?  out[i] is RB_OCCL_OCCLUDED exactly when the closest-hit search above would record a
 * hit if it were restricted to the stages named in `mask` and started with closest_hit.t = min(tmax[i], 1e20f) instead of 1e20f.
 * Everything else is that search's: `t > 0.001`, strict `<`, the device's normalisation of `dir`, the phantom light of an empty
 * light buffer (part of RB_MASK_LIGHTS), kept counts, numerics contract.  The reference's tree walk decides which triangles it
 * tests from boolean box tests only (shader.wgsl:282-392), so with RB_MASK_ALL the answer is rb_cast_rays(...).t < tmax[i].
 * The walk stops at the first accepted hit; the stages run ground, lights, spheres, triangles (the answer is existential).
 * The side effects are a query's: none on the accumulation, the frames, the colour buffer, the work counters or the random
 * sequence; rb_last_query_kernel_name reports "k_occl", "k_occl_bvh" or "k_occl_chunk", rb_last_query_ms their time. */
enum { RB_OCCL_VISIBLE = 0, RB_OCCL_OCCLUDED = 1, RB_OCCL_INVALID = 255 };
enum { RB_MASK_GROUND = 1, RB_MASK_TRIANGLES = 2, RB_MASK_SPHERES = 4, RB_MASK_LIGHTS = 8, RB_MASK_ALL = 15 };
/* n rays from host memory, tmax[n] (NULL: 1e20f for every ray), out[n] bytes (pageable or page-locked).  A ray rb_cast_rays
 * would mark RB_HIT_INVALID, or one whose tmax is NaN, is RB_OCCL_INVALID; tmax <= 0.001f (negative and -Inf included) is
 * VISIBLE and not walked; tmax >= 1e20f or +Inf is walked as 1e20f; mask == 0 makes every valid ray VISIBLE; mask bits above
 * RB_MASK_ALL and n > 2^31 - 64 are RB_ERR_INVALID_OPTIONS; n == 0 is RB_OK.  Pieces of at most 2^22 rays through the scratch
 * of rb_cast_rays' rays plus 16 MiB of bounds and 4 MiB of result bytes; the read-back is 1 B per ray. */
int rb_occluded(rb_engine* e, const rb_ray* rays, const float* tmax, size_t n, uint32_t mask, uint8_t* out);
/* The same with every pointer in device memory of the engine's device (a multi-device handle: devices[0]); a host pointer or
 * memory of another device is RB_ERR_INVALID_OPTIONS, and so are a d_rays that is not 16-byte aligned and a buffer whose
 * allocation (hipMemGetAddressRange) ends before its n elements.  The kernels are queued
 * on the engine's stream and read and write the caller's buffers directly -- no scratch, no copy, one launch unless the grid
 * limit demands more -- and the call returns without waiting: rb_sync is the wait.  The caller orders its own writes of the
 * buffers before the call.  rb_last_query_ms waits for the kernels it reports. */
int rb_occluded_device(rb_engine* e, const rb_ray* d_rays, const float* d_tmax, size_t n, uint32_t mask, uint8_t* d_out);
/* rb_cast_rays with d_rays, d_hits and d_surf (may be NULL) in device memory, 16-byte aligned; otherwise as rb_occluded_device.
 * On a sharded engine rays are whole-scene rays, as for rb_cast_rays. */
int rb_cast_rays_device(rb_engine* e, const rb_ray* d_rays, size_t n, rb_hit* d_hits, rb_surface* d_surf);

/* ---- Path-traced radiance along caller-given rays (the oracle's rbo_trace_ray).  For ray i of n and
 * sample k of `samples`:
 *   d_i       = normalize(dir_i) on the device, exactly as rb_cast_rays does it (the walks' margins need |d| = 1 +- 4 ulp);
 *   sid_i     = seeds ? seeds[i] : (uint32_t)i;
 *   seed(i,k) = pcg(sid_i + pcg(first_sample + k)) with u32 wrap-around: the first line of the shader's main with sid_i in
 *               place of pixel_index.  No jitter draws follow: the ray is the caller's;
 *   c(i,k)    = trace_ray(scene, origin_i, d_i, seed(i,k)), shader.wgsl:522-662: same max_depth, category order and strict
 *               `<`, phantom light, kept counts, colour hash and numerics contract as a render of the uploaded scene;
 *   out[i]    = {sum r, sum g, sum b, w}: the sum starts at +0.0f and adds c(i,0), c(i,1), ... in ascending k, one binary32
 *               add per component per sample; w = (float)samples.
 * A ray rb_cast_rays would mark RB_HIT_INVALID is not walked and yields {0, 0, 0, 0}; max_depth == 0 yields {0, 0, 0, samples}.
 * The side effects are a query's: none on the accumulation, the frames or the work counters (rb_get_stats does not move),
 * rb_last_kernel_name is unchanged and a pass the iterator has started ahead stays valid.  rb_last_query_kernel_name reports
 * "k_rad", "k_rad_bvh" or "k_rad_chunk" -- the walk by rb_cast_rays' rule -- and rb_last_query_ms their time with the sums'. */
typedef struct rb_radiance { float sum[3]; float weight; } rb_radiance;                              /* 16 B */
/* (ray, sample) items per launch: the colour scratch is 16 B x this (256 MiB) whatever n and samples are: a launch of this size
 * runs for milliseconds, so the tail every piece ends in stays a few per cent */
#define RB_TRACE_PIECE_ITEMS (1u << 24)
/* n rays and, unless NULL, n seeds from host memory; out[n] (pageable or page-locked).  RB_ERR_INVALID_OPTIONS, before any
 * launch: samples == 0 or > 65536, first_sample + samples beyond 2^32 - 1, n > 2^31 - 64, NULL rays or out with n > 0.
 * n == 0 is RB_OK.  The rays go through the device in pieces of at most RB_TRACE_PIECE_ITEMS items -- whole rays: a piece
 * never splits one ray's samples -- each launched, summed and copied out before the next.  The result does not depend on
 * the piece size, the launch shape or the form of the call.  Sharded engines and multi-device handles as rb_cast_rays. */
int rb_trace_rays(rb_engine* e, const rb_ray* rays, const uint32_t* seeds, size_t n, uint32_t first_sample, uint32_t samples,
                  rb_radiance* out);
/* The same with every pointer in device memory of the engine's device, validated as rb_occluded_device validates its buffers
 * (d_rays and d_out 16-byte aligned, d_seeds 4-byte).  Every launch is queued on the engine's stream and the call returns
 * without waiting: rb_sync is the wait. */
int rb_trace_rays_device(rb_engine* e, const rb_ray* d_rays, const uint32_t* d_seeds, size_t n, uint32_t first_sample,
                         uint32_t samples, rb_radiance* d_out);

/* ---- Camera rays made on the device (the normative definition; no reference counterpart).  A device stage
 * makes the ray of every (pixel, sample) item from the item's own random stream -- sub-pixel jitter, a fresh lens point per
 * sample -- and the kernels of rb_trace_rays trace it.  Every step is one IEEE binary32 operation in the order written, no
 * contraction, / and sqrt correctly rounded: the numpy model renderbaby_amd/camera.py equals the device bit for bit.
 * Pixel p = row * width + col, row 0 on top, column 0 on the left as the viewer sees it (no x mirror).  For pixel p and
 * sample k of `samples`:
 *   seed   = pcg(p + pcg(first_sample + k)), u32 wrap-around;
 *   jx, jy = random_float(&seed) - 0.5, twice; both always drawn, under RB_CAM_NO_JITTER both replaced by +0 after the draw;
 *   sx     = ((((float)col + 0.5f) + jx) / (float)width) * 2.0f - 1.0f;
 *   sy     = 1.0f - ((((float)row + 0.5f) + jy) / (float)height) * 2.0f;
 *   PERSPECTIVE  a = tan_half_fov * ((float)width / (float)height);  d0 = ((sx a) right + (sy tan_half_fov) up) + forward;
 *                lens_radius == 0: origin pos, direction d0, no further draw.  Otherwise lx = random_float 2 - 1, ly likewise,
 *                drawn again until lx lx + ly ly < 1;  o = (pos + (lens_radius lx) right) + (lens_radius ly) up;
 *                f = pos + focus_distance d0 (a focal PLANE: d0's forward part is 1);  direction f - o;
 *   ORTHO        o = (pos + (sx half_width) right) + (sy half_height) up;  direction forward;
 *   EQUIRECT     origin pos; (sin, cos) of longitude pi sx and latitude (pi / 2) sy from sincos_turn(sx) and
 *                sincos_turn(0.5f sy), the fixed polynomial routine of section 15.3 (within 2^-22 of the true values);
 *                d = ((cl sin lon) right + (sin lat) up) + (cl cos lon) forward, cl = cos lat;
 *   the direction is normalised as rb_cast_rays does it and the ray is invalid by rb_cast_rays' rule;
 *   c(p,k) = trace_ray(scene, o, d, seed) with the seed as the generator's draws left it;
 *   out[p - first_pixel] = {sum r, sum g, sum b, w}: from +0.0f in ascending k; w counts the valid samples; an invalid sample
 *   adds {0, 0, 0} with weight 0; max_depth == 0 gives {0, 0, 0, w}.
 * right, up and forward are used as given (the caller builds the basis).  The side effects are a query's.  The result does not
 * depend on the piece size, the launch shape or the form of the call. */
enum { RB_CAM_PERSPECTIVE = 1, RB_CAM_ORTHO = 2, RB_CAM_EQUIRECT = 3 };
enum { RB_CAM_NO_JITTER = 1u };
typedef struct rb_camera_ex {                                                                       /* 96 B */
    uint32_t kind, width, height, flags;
    float pos[3];     float tan_half_fov;    /* PERSPECTIVE: tan(fov_y / 2), made by the caller */
    float right[3];   float half_width;      /* ORTHO: half the window's width ... */
    float up[3];      float half_height;     /* ... and height */
    float forward[3]; float lens_radius;     /* PERSPECTIVE: 0 = pinhole */
    float focus_distance;                    /* PERSPECTIVE with a lens: distance of the focal plane along forward */
    uint32_t _reserved[3];                   /* must be 0 */
} rb_camera_ex;
/* (pixel, sample) items per launch of rb_trace_camera: 32 B of ray record and 16 B of colour each, 384 MiB of scratch */
#define RB_CAMERA_PIECE_ITEMS (1u << 23)
/* The generator alone, no engine, on `device` (-1 = current): rays_out / seeds_out[(p - first_pixel) * samples + k] in host
 * memory; rays_out[i].dir is normalised, an invalid ray has dir {0, 0, 0}; seeds_out[i] is the seed trace_ray starts with.
 * RB_ERR_INVALID_OPTIONS, before any device is touched: an unknown kind or flag bit; width or height 0 or above 2^24;
 * width * height >= 2^31; a pixel range that leaves the image; samples 0 or above 65536; first_sample + samples beyond
 * 2^32 - 1; n_pixels * samples above 2^31 - 64; a non-finite field; tan_half_fov <= 0, lens_radius < 0, focus_distance <= 0
 * with a lens (PERSPECTIVE); half_width or half_height <= 0 (ORTHO); non-zero _reserved.  NULL cam, rays_out or seeds_out with
 * n_pixels > 0: RB_ERR_NULL_ARGUMENT.  n_pixels == 0 is RB_OK. */
int rb_camera_rays(int32_t device, const rb_camera_ex* cam, uint64_t first_pixel, size_t n_pixels, uint32_t first_sample,
                   uint32_t samples, rb_ray* rays_out, uint32_t* seeds_out);
/* Radiance through the camera: out[n_pixels] in host memory (pageable or page-locked), pixels [first_pixel, first_pixel +
 * n_pixels) -- a tile or a region of the image.  Refusals as rb_camera_rays (NULL cam or out with n_pixels > 0:
 * RB_ERR_NULL_ARGUMENT); a refused call leaves the engine as it was.  Pieces of at most RB_CAMERA_PIECE_ITEMS items, whole
 * blocks of 64 pixels, never a part of one pixel's samples.  Sharded engines and multi-device handles as rb_trace_rays.
 * rb_last_query_kernel_name reports "k_cam", "k_cam_bvh" or "k_cam_chunk" -- the walk by rb_cast_rays' rule --,
 * rb_last_query_ms the generator, the trace and the sum together. */
int rb_trace_camera(rb_engine* e, const rb_camera_ex* cam, uint64_t first_pixel, size_t n_pixels, uint32_t first_sample,
                    uint32_t samples, rb_radiance* out);
/* The same with d_out in device memory of the engine's device, validated as rb_trace_rays_device validates its d_out; queued
 * on the engine's stream, returns without waiting: rb_sync is the wait. */
int rb_trace_camera_device(rb_engine* e, const rb_camera_ex* cam, uint64_t first_pixel, size_t n_pixels, uint32_t first_sample,
                           uint32_t samples, rb_radiance* d_out);
/* Measurement aid for tools/camera_rate.py (it may change or go): the share of k_cam_rays in the kernel time of the most recent
 * rb_trace_camera / rb_trace_camera_device, HIP events around the generator's launches, summed over the pieces, ms.  It waits
 * for the launches it reports. */
int rb_last_camera_rays_ms(rb_engine* e, float* ms);

/* ---- Hemisphere rays made on the device (the normative definition; no reference counterpart).  m surface
 * points in, m answers out: a device stage makes the cosine-weighted ray of every (surfel, sample) item from the item's own
 * random stream, and the kernels of rb_trace_rays (radiance) or rb_occluded (openness) walk it.  Every step is one IEEE binary32
 * operation in the order written, no contraction, / and sqrt correctly rounded: the numpy model renderbaby_amd/hemisphere.py
 * equals the device bit for bit.  For surfel i of n and sample k of `samples`:
 *   nrm    = normalize(normal_i) as rb_cast_rays normalises a direction; the surfel is invalid if pos_i or nrm has a non-finite
 *            component or nrm is all zero, and then so is every sample of it;
 *   sid    = seeds ? seeds[i] : (uint32_t)i;  seed = pcg(sid + pcg(first_sample + k)), u32 wrap-around: rb_trace_rays' rule;
 *   u1, u2 = random_float(&seed), twice: always exactly two draws, either may be exactly 1.0f;
 *   (s, c) = sincos_turn(u1 * 2.0f - 1.0f) (section 15.3);  r = sqrt(u2);  z = sqrt(1.0f - u2);
 *   sg = copysignf(1.0f, nrm.z);  a = -1.0f / (sg + nrm.z);  b = (nrm.x * nrm.y) * a;      (Duff et al. 2017; |sg + nrm.z| >= 1)
 *   t1 = (1.0f + (sg * (nrm.x * nrm.x)) * a,  sg * b,  (-sg) * nrm.x);   t2 = (b,  sg + (nrm.y * nrm.y) * a,  -nrm.y);
 *   d  = ((r * c) t1 + (r * s) t2) + z nrm, component-wise, then normalised as rb_cast_rays does it;
 *   reach = sqrt((px px + py py) + pz pz);  o = pos + (offset * max(1.0f, reach)) nrm;
 *   a sample is also invalid if o or d is non-finite or d is all zero.  An invalid item's record is {pos_i as given, 0 0 0};
 *   RADIANCE  c(i,k) = trace_ray(scene, o, d, seed) with the seed as the two draws left it; out[i] = {sum r, sum g, sum b, w}:
 *             from +0.0f in ascending k; w counts the valid samples; an invalid sample adds nothing; max_depth == 0 gives
 *             {0, 0, 0, w}.  The mean radiance sum / w is the irradiance over pi;
 *   OPENNESS  valid = the valid samples; open = those of them whose ray rb_occluded reports RB_OCCL_VISIBLE with tmax = radius
 *             and `mask` (radius <= 0.001f: every valid sample is open and nothing is walked).
 * The side effects are a query's.  The result does not depend on the piece size, the launch shape or the form of the call. */
typedef struct rb_surfel { float pos[3]; float _pad0; float normal[3]; float _pad1; } rb_surfel;    /* 32 B, rb_ray's layout */
/* (surfel, sample) items per launch, as RB_CAMERA_PIECE_ITEMS */
enum { RB_HEMI_PIECE_ITEMS = 1u << 23 };
typedef struct rb_hemi_params {                                                                     /* 32 B */
    float offset;      /* >= 0, finite: the origin leaves the surface by offset * max(1, |pos|) along the normal */
    float radius;      /* openness only: the any-hit bound, rb_occluded's tmax rules (NaN refused here) */
    uint32_t mask;     /* openness only: RB_MASK_* */
    uint32_t flags;    /* must be 0 */
    uint32_t _reserved[4];
} rb_hemi_params;
typedef struct rb_openness { uint32_t open; uint32_t valid; } rb_openness;                          /* 8 B */
/* The generator alone, no engine, on `device` (-1 = current): host arrays; rays_out / seeds_out[i * samples + k] as
 * rb_camera_rays writes them (dir normalised, an invalid ray {0, 0, 0}; the seed trace_ray starts with); `radius` and `mask`
 * are not read.  RB_ERR_INVALID_OPTIONS, before any device is touched: samples 0 or above 65536; first_sample + samples beyond
 * 2^32 - 1; n > 2^31 - 64 or n * samples above 2^31 - 64; offset negative or non-finite; non-zero flags or _reserved.  NULL
 * surfels, params, rays_out or seeds_out with n > 0: RB_ERR_NULL_ARGUMENT.  n == 0 is RB_OK. */
int rb_hemisphere_rays(int32_t device, const rb_surfel* surfels, const uint32_t* seeds, size_t n, const rb_hemi_params* params,
                       uint32_t first_sample, uint32_t samples, rb_ray* rays_out, uint32_t* seeds_out);
/* Radiance over the hemisphere: surfels[n], seeds[n] (may be NULL) and out[n] in host memory (pageable or page-locked).
 * Refusals as rb_hemisphere_rays; a refused call leaves the engine as it was.  Pieces of at most RB_HEMI_PIECE_ITEMS items,
 * whole blocks of 64 surfels, never a part of one surfel's samples.  Sharded engines and multi-device handles as
 * rb_trace_rays.  rb_last_query_kernel_name reports "k_cam", "k_cam_bvh" or "k_cam_chunk" -- the walk by rb_cast_rays' rule --,
 * rb_last_query_ms the generator, the trace and the sum together, rb_last_camera_rays_ms the generator's share. */
int rb_trace_hemisphere(rb_engine* e, const rb_surfel* surfels, const uint32_t* seeds, size_t n, const rb_hemi_params* params,
                        uint32_t first_sample, uint32_t samples, rb_radiance* out);
/* The same with d_surfels (16-byte aligned), d_seeds (may be NULL) and d_out in device memory of the engine's device, validated
 * as rb_trace_rays_device validates its buffers; queued on the engine's stream, returns without waiting: rb_sync is the wait. */
int rb_trace_hemisphere_device(rb_engine* e, const rb_surfel* d_surfels, const uint32_t* d_seeds, size_t n,
                               const rb_hemi_params* params, uint32_t first_sample, uint32_t samples, rb_radiance* d_out);
/* Openness: out[n] = {open, valid}.  As rb_trace_hemisphere, and RB_ERR_INVALID_OPTIONS for a NaN radius or mask bits above
 * RB_MASK_ALL.  The records, 4 B of bound and 1 B of result per item go through the engine's query scratch;
 * rb_last_query_kernel_name reports "k_occl", "k_occl_bvh" or "k_occl_chunk". */
int rb_openness_hemisphere(rb_engine* e, const rb_surfel* surfels, const uint32_t* seeds, size_t n, const rb_hemi_params* params,
                           uint32_t first_sample, uint32_t samples, rb_openness* out);
/* The same on device memory, as rb_trace_hemisphere_device (d_out: 8-byte aligned). */
int rb_openness_hemisphere_device(rb_engine* e, const rb_surfel* d_surfels, const uint32_t* d_seeds, size_t n,
                                  const rb_hemi_params* params, uint32_t first_sample, uint32_t samples, rb_openness* d_out);

/* ---- Lightmap texels made on the device (the normative definition; no reference counterpart).  The
 * triangles of a mesh are rasterised in uv space into an atlas of width x height texels, texel (x, y) = index y * width + x,
 * row 0 on TOP (sample_texture flips v, shader.wgsl:178-179); every owned texel becomes a surfel, the surfels are traced by
 * rb_trace_hemisphere's kernels and the sums resolved into a map in sample_texture's own layout.  Every step is one IEEE
 * binary32 operation in the order written, no contraction, / correctly rounded: the numpy model renderbaby_amd/lightmap.py
 * equals the device bit for bit.  For triangle t of bvh_triangles with uv indices i0, i1, i2:
 *   uv_k  = (uv_at(2 i_k), uv_at(2 i_k + 1)), u32 index arithmetic, out of range reads 0.0f (shader.wgsl:357-359);
 *   A, B, C = (u_k * float(width), (1.0f - v_k) * float(height));  P = (float(x) + 0.5f, float(y) + 0.5f);
 *   edge(S, T) at P: (a, b) = (S, T) if S.x < T.x || (S.x == T.x && S.y <= T.y), else (T, S);
 *            E = (b.x - a.x) * (P.y - a.y) - (b.y - a.y) * (P.x - a.x);  the value is E for ends in order, else -E;
 *   area = edge(A, B) at C;  w0 = edge(B, C), w1 = edge(C, A), w2 = edge(A, B) at P;
 *   box   x in [floor(min(A.x, B.x, C.x)), floor(max(A.x, B.x, C.x))], y likewise, cut to the atlas;
 *   COVER t covers nothing if the walks skip it (t >= bvh_triangle_count), its mesh_index is not params.mesh (unless that is
 *         RB_LIGHTMAP_ALL_MESHES), a coordinate of A, B, C is non-finite, or area is zero or non-finite; else it covers the
 *         texels of its box with w0, w1, w2 all >= 0 (area > 0) or all <= 0 (area < 0): zero counts as inside;
 *   OWNER the lowest covering triangle index, or RB_LIGHTMAP_NO_OWNER;
 *   SURFEL of an owned texel: u = w1 / area; v = w2 / area; pos = (v0 + u e1) + v e2, component-wise, e1 = v1 - v0,
 *         e2 = v2 - v0; normal = normalize(cross(e1, e2)) as the walks report it, every component negated with
 *         RB_LIGHTMAP_FLIP; pad words 0.  An unowned texel's surfel is all zero bits: rb_trace_hemisphere's invalid surfel;
 *   RESOLVE sums[n] -> rgba[n]: pass 0: sums.w > 0 ? {r / w, g / w, b / w, 1.0f} : {0, 0, 0, 0}; then `dilate` passes, each
 *         reading the pass before only: a texel whose fourth component is 0 sums, from +0.0f and in the order (-1,-1) (0,-1)
 *         (1,-1) (-1,0) (1,0) (-1,1) (0,1) (1,1) of (dx, dy), its neighbours inside the atlas with a non-zero fourth
 *         component; c > 0 of them make it {sum r / float(c), sum g / float(c), sum b / float(c), 2.0f}.
 *         Fourth component: 0 = empty, 1 = baked, 2 = filled.
 * The result depends on neither the launch shape nor the form of the call. */
enum { RB_LIGHTMAP_ALL_MESHES = 0xFFFFFFFFu, RB_LIGHTMAP_NO_OWNER = 0xFFFFFFFFu, RB_LIGHTMAP_FLIP = 1u };
enum { RB_LIGHTMAP_MAX_SIDE = 16384u, RB_LIGHTMAP_MAX_DILATE = 64u };
typedef struct rb_lightmap_params {   /* 32 B */
    uint32_t width, height;   /* 1 .. 16384 each; width * height <= 2^31 - 64 */
    uint32_t mesh;            /* mesh index or RB_LIGHTMAP_ALL_MESHES */
    uint32_t flags;           /* RB_LIGHTMAP_FLIP or 0 */
    float    offset;          /* handed to rb_hemi_params.offset: >= 0, finite */
    uint32_t dilate;          /* 0 .. 64 passes */
    uint32_t _reserved[2];    /* must be 0 */
} rb_lightmap_params;
/* The generator alone, no engine, on `device` (-1 = current): host arrays.  The triangles are prepared by the device code of
 * the engine's upload, so the normals are the engine's; every triangle counts as valid.  surfels_out[width * height],
 * owners_out[width * height] (may be NULL).  RB_ERR_NULL_ARGUMENT: NULL params or surfels_out, NULL tris with n_tris > 0, NULL
 * uvs with n_uv_floats > 0.  RB_ERR_INVALID_OPTIONS, before any device is touched: width or height 0 or above 16384; width *
 * height above 2^31 - 64; dilate above 64; unknown flags; non-zero _reserved; offset negative or non-finite; n_tris above
 * 2^31 - 64 or n_uv_floats above 2^32 - 1.  n_tris == 0 is RB_OK with an all-empty map, and no device is touched. */
int rb_lightmap_surfels(int32_t device, const rb_gpu_triangle* tris, size_t n_tris, const float* uvs, size_t n_uv_floats,
                        const rb_lightmap_params* params, rb_surfel* surfels_out, uint32_t* owners_out);
/* From the engine's uploaded scene into device memory of the engine's device (d_surfels: 16-byte aligned, width * height
 * records; d_owners: may be NULL), validated as rb_trace_rays_device validates its buffers.  Queued on the engine's stream; the
 * call waits once, for the 8 bytes that size the cover launches, and returns without waiting for the rest: rb_sync is the wait.
 * The result is what rb_trace_hemisphere_device and rb_openness_hemisphere_device take.  The side effects are a query's. */
int rb_lightmap_surfels_device(rb_engine* e, const rb_lightmap_params* params, rb_surfel* d_surfels, uint32_t* d_owners);
/* The resolve alone, no engine, on `device` (-1 = current): sums[width * height] -> rgba_out[width * height * 4], host arrays.
 * Refusals as above for width, height and dilate; NULL sums or rgba_out: RB_ERR_NULL_ARGUMENT. */
int rb_lightmap_resolve(int32_t device, uint32_t width, uint32_t height, const rb_radiance* sums, uint32_t dilate, float* rgba_out);
/* The bake: surfels (in the engine's query scratch), rb_trace_hemisphere's pieces over them with seeds = NULL -- the stream id
 * is the texel index --, resolve.  rgba_out[width * height * 4] and sums_out[width * height] (the raw sums, for a caller who
 * accumulates over calls with first_sample and resolves later) in host memory; either may be NULL, not both.  The limits on
 * width * height * samples are rb_trace_hemisphere's and refuse the same way.  An engine without triangles, or an atlas no
 * triangle covers, is RB_OK with an all-empty map.  Sharded engines and multi-device handles as rb_trace_rays.
 * rb_last_query_ms reports all three stages, rb_last_lightmap_ms the first and the last. */
int rb_bake_lightmap(rb_engine* e, const rb_lightmap_params* params, uint32_t first_sample, uint32_t samples, float* rgba_out,
                     rb_radiance* sums_out);
/* The same into device memory of the engine's device (16-byte aligned), as rb_lightmap_surfels_device. */
int rb_bake_lightmap_device(rb_engine* e, const rb_lightmap_params* params, uint32_t first_sample, uint32_t samples,
                            float* d_rgba_out, rb_radiance* d_sums_out);
/* Kernel ms of the surfel stage (prepare, count, scan, cover, surfels) and of the resolve (with its dilate passes) in the most
 * recent lightmap call; a stage the call did not run reports 0.  Either pointer may be NULL. */
int rb_last_lightmap_ms(rb_engine* e, float* surfels_ms, float* resolve_ms);

/* ---- Irradiance probes made on the device (the normative definition; no reference counterpart).  n points
 * in free space in, n records of SH9 sums out -- nine real spherical-harmonic coefficients (bands 0-2) per colour channel of
 * the radiance arriving from every direction: a device stage makes the uniform-sphere ray of every (probe, sample) item from
 * the item's own random stream, the kernels of rb_trace_rays walk it, and a second stage folds each item's colour with the
 * basis of the item's own direction.  Every step is one IEEE binary32 operation in the order written, no contraction, / and
 * sqrt correctly rounded: the numpy model renderbaby_amd/probes.py equals the device bit for bit.  For probe i of n and sample
 * k of `samples`:
 *   pos    = probes[i].pos; the probe is invalid if a component is non-finite, and then so is every sample of it;
 *   sid    = seeds ? seeds[i] : (uint32_t)i;  seed = pcg(sid + pcg(first_sample + k)), u32 wrap-around: rb_trace_rays' rule;
 *   u1, u2 = random_float(&seed), twice: always exactly two draws, either may be exactly 1.0f;
 *   (s, c) = sincos_turn(u1 * 2.0f - 1.0f) (section 15.3);  z = 1.0f - (u2 + u2);  r = sqrt(1.0f - z * z);
 *   d      = (r * c, r * s, z) normalised as rb_cast_rays does it: world axes, no frame;  the origin is pos, no offset;
 *   a sample is invalid by rb_cast_rays' rule, and its record is {pos as given, 0 0 0};
 *   c(i,k) = trace_ray(scene, pos, d, seed) with the seed as the two draws left it;
 *   Y0 = 0.282094792f;  Y1 = 0.488602512f * d.y;  Y2 = 0.488602512f * d.z;  Y3 = 0.488602512f * d.x;
 *   Y4 = 1.09254843f * (d.x * d.y);  Y5 = 1.09254843f * (d.y * d.z);  Y6 = 0.315391565f * (3.0f * (d.z * d.z) - 1.0f);
 *   Y7 = 1.09254843f * (d.x * d.z);  Y8 = 0.546274215f * (d.x * d.x - d.y * d.y), d as stored in the item's record;
 *   out[i].sum[j][ch]: from +0.0f in ascending k, += c(i,k)[ch] * Yj (one multiply, one add); out[i].weight counts the valid
 *   samples; an invalid sample leaves every sum's bits as they were; max_depth == 0 gives all-zero sums with the weight set.
 * The radiance coefficient is L_j = (4 pi / weight) sum[j]: the division is the caller's, so that sums can be accumulated over
 * calls with first_sample.  The side effects are a query's.  The result does not depend on the piece size, the launch shape or
 * the form of the call. */
typedef struct rb_probe { float pos[3]; float _pad; } rb_probe;                                     /* 16 B */
typedef struct rb_sh9 { float sum[9][3]; float weight; } rb_sh9;                                    /* 112 B */
/* (probe, sample) items per launch, as RB_HEMI_PIECE_ITEMS */
enum { RB_PROBE_PIECE_ITEMS = 1u << 23 };
/* The generator alone, no engine, on `device` (-1 = current): host arrays; rays_out[i * samples + k] as rb_hemisphere_rays
 * writes it, and the seed trace_ray starts with in seeds_out[i * samples + k] or, with seeds_out NULL, as the bits of the
 * record's fourth word.  RB_ERR_INVALID_OPTIONS, before any device is touched: samples 0 or above 65536; first_sample + samples
 * beyond 2^32 - 1; n > 2^31 - 64 or n * samples above 2^31 - 64.  NULL probes or rays_out with n > 0: RB_ERR_NULL_ARGUMENT.
 * n == 0 is RB_OK. */
int rb_probe_rays(int32_t device, const rb_probe* probes, const uint32_t* seeds, size_t n, uint32_t first_sample, uint32_t samples,
                  rb_ray* rays_out, uint32_t* seeds_out);
/* The bake: probes[n], seeds[n] (may be NULL) and out[n] in host memory (pageable or page-locked).  Refusals as rb_probe_rays
 * (NULL probes or out with n > 0: RB_ERR_NULL_ARGUMENT); a refused call leaves the engine as it was.  Pieces of at most
 * RB_PROBE_PIECE_ITEMS items, whole blocks of 64 probes, never a part of one probe's samples.  Sharded engines and multi-device
 * handles as rb_trace_rays.  rb_last_query_kernel_name reports "k_cam", "k_cam_bvh" or "k_cam_chunk" -- the walk by
 * rb_cast_rays' rule --, rb_last_query_ms the generator, the trace and the projection together, rb_last_camera_rays_ms the
 * generator's share. */
int rb_bake_probes(rb_engine* e, const rb_probe* probes, const uint32_t* seeds, size_t n, uint32_t first_sample, uint32_t samples,
                   rb_sh9* out);
/* The same with d_probes and d_out (16-byte aligned) and d_seeds (may be NULL) in device memory of the engine's device,
 * validated as rb_trace_rays_device validates its buffers; queued on the engine's stream, returns without waiting: rb_sync is
 * the wait. */
int rb_bake_probes_device(rb_engine* e, const rb_probe* d_probes, const uint32_t* d_seeds, size_t n, uint32_t first_sample,
                          uint32_t samples, rb_sh9* d_out);

/* Measurement aid for tools/probe_rate.py (it may change or go): the share of the projection in the kernel time of the most
 * recent rb_bake_probes / rb_bake_probes_device, HIP events around its launches, summed over the pieces, ms.  It waits for the
 * launches it reports. */
int rb_last_probe_project_ms(rb_engine* e, float* ms);

/* ---- Light points from a baked probe grid (the normative definition; no reference counterpart).  The
 * way back in for what rb_bake_probes makes: a regular axis-aligned grid of probes and m points with normals in, m lit values
 * out.  Every step is one IEEE binary32 operation in the order written, no contraction, / and sqrt correctly rounded: the numpy
 * model renderbaby_amd/probes.py (coefficients, light) equals the device bit for bit -- but for the sign and payload of a NaN
 * the arithmetic itself generates.  max(x, 0.0f) is x > 0.0f ? x : 0.0f and min(x, y) is x < y ? x : y.
 *   GRID   probe (ix, iy, iz) sits at origin + i * step, its record at index (iz * ny + iy) * nx + ix, x fastest.
 *   COEFFS (stage 1, one record each): a probe is valid if its weight is finite and > 0.  Valid: coeff[j][ch] = (sum[j][ch] *
 *          K_j) / weight with K_0 = 12.566371f (4 pi), K_1..3 = 8.37758f (8 pi / 3), K_4..8 = 3.1415927f (pi) -- 4 A_l, the
 *          cosine lobe's zonal factors, so that sum_j coeff_j Y_j(n) is the irradiance over pi --, and the weight word becomes
 *          1.0f.  Invalid: all-zero bits.  The output may be the input.
 *   LIGHT  (stage 2) for point i with pos and nrm:
 *          invalid point: a non-finite component of pos or nrm, nrm all zero, or (nx nx + ny ny) + nz nz not finite: {0, 0, 0, 0};
 *          n = nrm / sqrt((nx nx + ny ny) + nz nz), as rb_cast_rays normalises;  Y0..Y8 = rb_bake_probes' basis of n;
 *          per axis a: f = (pos_a - origin_a) / step_a;  f = min(max(f, 0.0f), float(count_a - 1));
 *                      i_a = min(uint(floor(f)), count_a >= 2 ? count_a - 2 : 0);  t_a = f - float(i_a);
 *          the corners (ix + dx, iy + dy, iz + dz) in the order dz, dy, dx ascending, dx fastest; a corner with d_a = 1 on an
 *          axis with count_a == 1 does not exist;  w_c = ((wx * wy) * wz) * coeff[c].weight, w_a = d_a ? t_a : 1.0f - t_a;
 *          a corner that does not exist or whose w_c == 0 is skipped: no value of its record enters the arithmetic;
 *          e_c[ch]: from +0.0f, j ascending, += coeff[c][j][ch] * Yj (one multiply, one add);
 *          E[ch] += w_c * e_c[ch] and W += w_c, from +0.0f in corner order;
 *          out = W > 0 ? {max(E.r / W, 0.0f), max(E.g / W, 0.0f), max(E.b / W, 0.0f), W} : {0, 0, 0, 0}.
 * `value` is the irradiance over pi -- what rb_trace_hemisphere's sum / weight estimates --, so albedo x value is a lambert
 * surface's outgoing radiance.  A point outside the grid takes the values at the nearest cell's edge.  A caller rejects a probe
 * (one inside geometry, say) by zeroing its weight before stage 1: the blend renormalises over the rest.  Visibility and backface
 * weights against leaks, and what finds such a probe: rb_light_points_visible below (section 20).  Not here: anything but a
 * regular axis-aligned grid. */
typedef struct rb_probe_grid {                                                                      /* 48 B */
    float origin[3];      /* finite */
    uint32_t _pad0;       /* must be 0 */
    float step[3];        /* finite, > 0 */
    uint32_t _pad1;       /* must be 0 */
    uint32_t counts[3];   /* nx, ny, nz: each >= 1, nx * ny * nz <= 2^31 - 64 */
    uint32_t flags;       /* must be 0 */
} rb_probe_grid;
typedef struct rb_lit { float value[3]; float weight; } rb_lit;                                     /* 16 B */
/* Stage 1 alone, no engine, on `device` (-1 = current): sums[n] -> coeffs_out[n], host arrays (coeffs_out may be sums).  n above
 * 2^31 - 64: RB_ERR_INVALID_OPTIONS; NULL sums or coeffs_out with n > 0: RB_ERR_NULL_ARGUMENT; both before any device is
 * touched.  n == 0 is RB_OK. */
int rb_probe_coefficients(int32_t device, const rb_sh9* sums, size_t n, rb_sh9* coeffs_out);
/* The same with d_sums and d_coeffs_out (16-byte aligned; they may be the same buffer) in device memory of the engine's device,
 * validated as rb_trace_rays_device validates its buffers; queued on the engine's stream, returns without waiting: rb_sync is
 * the wait.  The engine lends its device and its stream: no scene is read, and the side effects are a query's -- none.  Like
 * every engine entry point it asks for an engine that holds a scene: before the first rb_update it is RB_ERR_NOT_INITIALIZED,
 * with n == 0 too.  Sharded engines and multi-device handles as rb_trace_rays (a multi-device handle answers on devices[0]).
 * rb_last_query_ms reports the kernel, rb_last_query_kernel_name "k_probe_coeffs". */
int rb_probe_coefficients_device(rb_engine* e, const rb_sh9* d_sums, size_t n, rb_sh9* d_coeffs_out);
/* Stage 2, no engine, on `device` (-1 = current): the grid, its nx * ny * nz coefficient records, points[m] and out[m] in host
 * memory.  The records are uploaded once; the points go through the device in pieces of 2^22 (RB_LIGHT_PIECE_POINTS in the
 * environment, read per call: another piece size, for tests); the result does not depend on it.  RB_ERR_NULL_ARGUMENT: a NULL
 * grid; NULL coeffs, points or out with m > 0.  RB_ERR_INVALID_OPTIONS, before any device is touched: a count of 0; nx * ny * nz
 * above 2^31 - 64; m above 2^31 - 64; a step that is not finite or not > 0; a non-finite origin; non-zero flags or pad words.
 * m == 0 is RB_OK. */
int rb_light_points(int32_t device, const rb_probe_grid* grid, const rb_sh9* coeffs, const rb_surfel* points, size_t m, rb_lit* out);
/* The same with d_coeffs, d_points and d_out (16-byte aligned) in device memory of the engine's device; the grid itself is host
 * memory and is read before the call returns.  One launch, as rb_probe_coefficients_device in every other respect;
 * rb_last_query_kernel_name reports "k_probe_light" (or "k_probe_light_wide": RB_LIGHT_SHAPE=wide in the environment chooses the
 * other launch shape for a measurement; the result does not depend on it). */
int rb_light_points_device(rb_engine* e, const rb_probe_grid* grid, const rb_sh9* d_coeffs, const rb_surfel* d_points, size_t m,
                           rb_lit* d_out);

/* ---- Probe visibility: depth moments baked on the device, a leak-free blend (the normative definition;
 * no reference counterpart; after Majercik et al. 2019, "Dynamic Diffuse Global Illumination with Ray-Traced Irradiance
 * Fields").  Each probe keeps an 8 x 8 octahedral map of the mean and the mean square of the distance to the first hit; the
 * blend weighs every corner by a Chebyshev bound of the point's distance against them and by a wrapped cosine of the point's
 * normal towards the probe; the share of a probe's rays that met a back face tells which probes sit inside geometry.  Every
 * step is one IEEE binary32 operation in the order written, no contraction, / and sqrt correctly rounded: the numpy model
 * renderbaby_amd/probes.py (oct_texel, depth_project, moments, light_visible) equals the device bit for bit -- but for the sign
 * and payload of a NaN the arithmetic itself generates.  max(x, y) is x > y ? x : y and min(x, y) is x < y ? x : y.  Points so
 * far from the grid that a difference of positions overflows are outside the contract (nothing is read out of bounds).
 *   TEXEL  oct_texel(v), v any non-zero vector, not normalised:
 *          s = (|vx| + |vy|) + |vz|;  px = vx / s;  py = vy / s;
 *          if vz < 0.0f: (px, py) = ((1.0f - |py|) * sgn(px), (1.0f - |px|) * sgn(py)) with the old px, py on the right,
 *          sgn(x) = x >= 0.0f ? 1.0f : -1.0f  (vz == -0.0f stays in the upper half);
 *          tx = min(uint(floor((px * 0.5f + 0.5f) * 8.0f)), 7), ty likewise from py;  T = ty * 8 + tx.  Nearest texel only.
 *   BAKE   probe i, sample k: the ray is rb_bake_probes' (same ids, first_sample and samples: the same record), the hit
 *          rb_cast_rays' of that record.  From all-zero bits, in ascending k: a sample whose stored direction is 0 0 0 or whose
 *          hit kind is RB_HIT_INVALID is skipped; else T = oct_texel(d as stored), r = min(hit.t, max_distance) (a miss has
 *          t = 1e20f: max_distance), texel[T] += {r, r * r, 1.0f, back} with back = 1.0f if the kind is RB_HIT_TRIANGLE or
 *          RB_HIT_SPHERE and (n.x d.x + n.y d.y) + n.z d.z > 0.0f, n = hit.normal, else the word stays as it is.
 *   MOMENTS per texel {sum_r, sum_r2, count, back}: count > 0 and finite: {sum_r / count, sum_r2 / count, 1.0f, back / count};
 *          else all-zero bits.  backface_share[i] = C == 0 ? 0.0f : B / C, B and C the sums of `back` and `count` over the
 *          texels in ascending order from +0.0f (sums of integers: below 2^24 samples any order gives the same bits).
 *   BLEND  rb_light_points' stage 2 with every existing corner's weight extended: tl = ((wx * wy) * wz) * coeff[c].weight;
 *          a corner with tl == 0 is skipped as there; else, per axis a, P_a = origin_a + float(i_a + d_a) * step_a;
 *          q = P - pos;  l = sqrt((qx qx + qy qy) + qz qz);  cw = l > 0.0f ? ((qx n.x + qy n.y) + qz n.z) / l : 1.0f;
 *          h = (cw + 1.0f) * 0.5f;  wb = h * h + 0.2f  (RB_VIS_NO_WRAP: wb = 1.0f);
 *          b_a = pos_a + n_a * normal_bias;  v = b - P;  r = sqrt((vx vx + vy vy) + vz vz);
 *          vis = 1.0f if RB_VIS_NO_DEPTH or r == 0.0f; else (mean, mean2, valid, _) = moments[c].texel[oct_texel(v)] and
 *          vis = 1.0f if valid == 0.0f or !(r > mean), else var = |mean2 - mean * mean|;  dl = r - mean;  den = var + dl * dl;
 *          ch = den > 0.0f ? var / den : 1.0f;  vis = (ch * ch) * ch;
 *          vis = max(vis, min_visibility);  w_c = (tl * wb) * vis;  a corner with w_c == 0 is skipped like one that does not
 *          exist.  E, W and the output are rb_light_points'.  With both flags w_c = tl: rb_light_points' result bit for bit. */
typedef struct rb_probe_depth { float texel[64][4]; } rb_probe_depth;     /* 1024 B; a texel: {sum_r, sum_r2, count, back} */
enum { RB_VIS_NO_WRAP = 1, RB_VIS_NO_DEPTH = 2 };
typedef struct rb_light_visibility {                                                                /* 16 B */
    float normal_bias;      /* finite: the point moves this far along its unit normal before the depth test */
    float min_visibility;   /* 0 .. 1: the floor of the depth weight */
    uint32_t flags;         /* RB_VIS_* */
    uint32_t _pad;          /* must be 0 */
} rb_light_visibility;
/* The depth bake: rb_bake_probes' arguments and max_distance in, out[n] raw sums (a caller may accumulate them over calls).
 * Refusals, pieces of whole probes (at most 2^22 items, whole blocks of 64 probes: the hit scratch is rb_cast_rays';
 * RB_DEPTH_PIECE_ITEMS in the environment, read per call: fewer items, for tests; the result does not depend on it), sharded
 * engines, multi-device handles and side effects (a query's: none) as rb_bake_probes; max_distance not finite or not > 0:
 * RB_ERR_INVALID_OPTIONS before any device is touched.  rb_last_query_kernel_name reports "k_query", "k_query_bvh" or
 * "k_query_chunk", rb_last_query_ms the generator, the query and the projection together, rb_last_camera_rays_ms the
 * generator's share.  RB_DEPTH_SHAPE=lds|readlane in the environment chooses the projection's other fold for a measurement;
 * the result does not depend on it. */
int rb_bake_probe_depth(rb_engine* e, const rb_probe* probes, const uint32_t* seeds, size_t n, uint32_t first_sample, uint32_t samples,
                        float max_distance, rb_probe_depth* out);
/* The same with d_probes and d_out (16-byte aligned) and d_seeds (may be NULL) in device memory of the engine's device; queued
 * on the engine's stream, returns without waiting: rb_sync is the wait. */
int rb_bake_probe_depth_device(rb_engine* e, const rb_probe* d_probes, const uint32_t* d_seeds, size_t n, uint32_t first_sample,
                               uint32_t samples, float max_distance, rb_probe_depth* d_out);
/* Measurement aid for tools/probe_visibility_rate.py (it may change or go): the projection's share of the kernel time of the
 * most recent rb_bake_probe_depth / _device, as rb_last_probe_project_ms. */
int rb_last_probe_depth_project_ms(rb_engine* e, float* ms);
/* MOMENTS, no engine, on `device` (-1 = current): sums[n] -> moments_out[n] (it may be sums) and, unless NULL,
 * backface_share_out[n]; host arrays.  n above 2^31 - 64: RB_ERR_INVALID_OPTIONS; NULL sums or moments_out with n > 0:
 * RB_ERR_NULL_ARGUMENT; both before any device is touched.  n == 0 is RB_OK. */
int rb_probe_moments(int32_t device, const rb_probe_depth* sums, size_t n, rb_probe_depth* moments_out, float* backface_share_out);
/* The same in device memory of the engine's device (16-byte aligned, the share 4-byte; d_moments_out may be d_sums), as
 * rb_probe_coefficients_device in every other respect; rb_last_query_kernel_name reports "k_probe_moments". */
int rb_probe_moments_device(rb_engine* e, const rb_probe_depth* d_sums, size_t n, rb_probe_depth* d_moments_out, float* d_backface_share_out);
/* BLEND, no engine: rb_light_points with the grid's nx * ny * nz moment maps (the records' order) and the parameters.  Refusals
 * as rb_light_points, and RB_ERR_NULL_ARGUMENT: NULL params; NULL moments with m > 0 unless RB_VIS_NO_DEPTH is set (they are not
 * read then); RB_ERR_INVALID_OPTIONS: normal_bias not finite, min_visibility outside [0, 1] or NaN, flag bits other than
 * RB_VIS_*, a non-zero pad.  Maps and records are uploaded once, the points go in rb_light_points' pieces. */
int rb_light_points_visible(int32_t device, const rb_probe_grid* grid, const rb_sh9* coeffs, const rb_probe_depth* moments,
                            const rb_surfel* points, size_t m, const rb_light_visibility* params, rb_lit* out);
/* The same in device memory of the engine's device, as rb_light_points_device; rb_last_query_kernel_name reports
 * "k_probe_light_vis". */
int rb_light_points_visible_device(rb_engine* e, const rb_probe_grid* grid, const rb_sh9* d_coeffs, const rb_probe_depth* d_moments,
                                   const rb_surfel* d_points, size_t m, const rb_light_visibility* params, rb_lit* d_out);

/* ---- Direct light at surface points: shadow rays to the scene's emitters, made on the device (the
 * normative definition; no reference counterpart).  rb_trace_hemisphere finds a light only when a cosine-weighted ray happens
 * to hit it; here every sample picks an emitter, draws a point on it and asks rb_occluded whether the segment is free.  Every
 * step is one IEEE binary32 operation in the order written, no contraction, / and sqrt correctly rounded: the numpy model
 * renderbaby_amd/direct.py (scene_emitters, rays, fold) equals the device bit for bit.
 *   TABLE  the scene's emitters: triangles t < bvh_triangle_count (the patched, clamped count a render sees) with mesh_index <
 *          the number of meshes, ascending; then spheres k < spheres_count; then lights k < arrayLength(lights).
 *          Triangle: a = v0, b = v1 - v0, c = v2 - v0, cr = cross(b, c), area = 0.5f * sqrt((cr.x cr.x + cr.y cr.y) + cr.z cr.z).
 *          Sphere or light: a = center, b = {radius, 0, 0}, c = 0, area = 12.566371f * (radius * radius), radius > 0.
 *          emissive = what rb_cast_rays reports in rb_surface.emissive for a hit on the primitive (a triangle under
 *          color_hash_enabled: 0).  A primitive qualifies when emissive is finite with its largest component > 0, a, b, c are
 *          finite and area is finite and > 0.  The phantom light of an empty light buffer never qualifies.
 *   ITEM   surfel i, sample k, N emitters.  nrm, sid, the validity of the surfel and o = pos + (offset * max(1.0f, reach)) nrm
 *          are rb_trace_hemisphere's; seed = pcg(sid + pcg(first_sample + k)); u0, u1, u2 = random_float(&seed), always three.
 *          j = min(uint(u0 * float(N)), N - 1), E = emitters[j]; E is bad if a, b, c, area or emissive is not finite, area <= 0
 *          or kind is none of RB_HIT_TRIANGLE / _SPHERE / _LIGHT.
 *          Triangle: su = sqrt(u1), bv = u2 * su, bu = su - bv, Q = (a + bu b) + bv c, ne = normalize(cross(b, c)).
 *          Else: (s, c) = sincos_turn(u1 * 2.0f - 1.0f), z = 1.0f - (u2 + u2), r = sqrt(1.0f - z * z), ne = (r * c, r * s, z),
 *          Q = a + b.x ne.
 *          v = Q - o, d2 = (v.x v.x + v.y v.y) + v.z v.z, dist = sqrt(d2), d = v / dist, cs = (nrm.x d.x + nrm.y d.y) + nrm.z d.z,
 *          ce likewise with ne, then |ce| for a triangle (it emits on both sides) and -ce otherwise (a sphere from outside only).
 *          The item is lit when the surfel is valid, N > 0, E is good, d is finite and not 0 0 0, cs > 0, ce > 0, d2 > 0 and
 *          contrib = emissive * g, g = ((((cs * ce) * area) / d2) * float(N)) * 0.318309886f, is finite in every component.
 *   OUT    per item the record {o, d} (pad words 0), the bound dist * (1.0f - shorten) if lit, else 0.0f (rb_occluded answers
 *          VISIBLE without walking), and {contrib if lit else +0, valid ? 1.0f : 0.0f}.  A valid item whose d is not finite
 *          stores d = 0 0 0; an invalid item stores {pos as given, 0 0 0}: rb_occluded marks both RB_OCCL_INVALID.
 *   FOLD   out[i].sum from +0, in ascending k: + contrib of every item whose byte is RB_OCCL_VISIBLE, one add per component;
 *          out[i].weight = the number of valid items.  sum / weight is the direct irradiance over pi: rb_trace_hemisphere's
 *          convention, so the two add and compare. */
typedef struct rb_emitter {                                                                        /* 64 B */
    float a[3]; uint32_t kind;    /* RB_HIT_TRIANGLE, RB_HIT_SPHERE or RB_HIT_LIGHT */
    float b[3]; uint32_t prim;    /* index into bvh_triangles / spheres / lights */
    float c[3]; float area;
    float emissive[3]; float _pad;
} rb_emitter;
typedef struct rb_light_params {                                                                   /* 32 B */
    float offset;           /* as rb_hemi_params' */
    float shorten;          /* finite, 0 .. 0.5: the shadow ray ends this fraction short of the sampled point */
    uint32_t mask;          /* RB_MASK_*: what may occlude */
    uint32_t flags;         /* must be 0 */
    uint32_t _reserved[4];  /* must be 0 */
} rb_light_params;
/* more emitters than this in a table: RB_ERR_INVALID_OPTIONS, so that float(N) is exact */
#define RB_MAX_EMITTERS (1u << 24)
/* TABLE of the engine's scene into host memory: min(*count, capacity) records are written (out may be NULL with capacity 0),
 * *count is always the total.  The table is made on the device -- flag, exclusive scan, scatter over the raw scene arrays --
 * by the first call that needs it after an rb_update and kept until the next one; that first call waits once, for the total
 * that sizes it.  A query in every other respect (rb_cast_rays' side effects: none; a multi-device handle: devices[0]);
 * rb_last_query_ms reports the kernel time of the build, 0 when the table stood.  NULL count: RB_ERR_NULL_ARGUMENT; more than
 * 2^31 - 64 candidates or more than RB_MAX_EMITTERS emitters: RB_ERR_INVALID_OPTIONS. */
int rb_scene_emitters(rb_engine* e, rb_emitter* out, size_t capacity, size_t* count);
/* The same into device memory of the engine's device: d_out (16-byte aligned, capacity records; may be NULL with capacity 0)
 * and d_count (one uint32_t, 4-byte aligned); queued on the engine's stream, nothing is waited for once the table stands. */
int rb_scene_emitters_device(rb_engine* e, rb_emitter* d_out, size_t capacity, uint32_t* d_count);
/* ITEM and OUT alone, no engine, on `device` (-1 = current), host arrays in LINEAR order: item i * samples + k is sample
 * first_sample + k of surfels[i]; rays_out, tmax_out and contrib_out (float4 per item) hold n * samples items each.  `seeds`:
 * the surfels' ids, or NULL: their indices.  Refusals as rb_hemisphere_rays (it reads no mask), and RB_ERR_INVALID_OPTIONS:
 * shorten not finite or outside [0, 0.5], n_emit > RB_MAX_EMITTERS; RB_ERR_NULL_ARGUMENT: NULL emitters with n_emit > 0, and
 * with n > 0 NULL surfels, params or outputs; all before any device is touched.  n == 0 is RB_OK. */
int rb_light_rays(int32_t device, const rb_emitter* emitters, size_t n_emit, const rb_surfel* surfels, const uint32_t* seeds, size_t n,
                  const rb_light_params* params, uint32_t first_sample, uint32_t samples, rb_ray* rays_out, float* tmax_out, float* contrib_out);
/* ITEM, rb_occluded over the records and bounds with params->mask, FOLD: out[n].  emitters == NULL: the scene's own table
 * (n_emit is ignored); else n_emit records of the caller's -- one light, or one group of lights, gets a map of its own.
 * Refusals (rb_light_rays', and a mask above RB_MASK_ALL), side effects, pieces of whole blocks of 64 surfels and at most
 * RB_HEMI_PIECE_ITEMS items, sharded engines and multi-device handles as rb_openness_hemisphere.  rb_last_query_kernel_name
 * reports "k_occl", "k_occl_bvh" or "k_occl_chunk", rb_last_query_ms the three stages together, rb_last_camera_rays_ms the
 * generator's share. */
int rb_direct_light(rb_engine* e, const rb_emitter* emitters, size_t n_emit, const rb_surfel* surfels, const uint32_t* seeds, size_t n,
                    const rb_light_params* params, uint32_t first_sample, uint32_t samples, rb_radiance* out);
/* The same with d_surfels, d_out and, when given, d_emitters (16-byte aligned) and d_seeds (may be NULL) in device memory of
 * the engine's device; validated and queued as rb_trace_hemisphere_device, returns without waiting: rb_sync is the wait. */
int rb_direct_light_device(rb_engine* e, const rb_emitter* d_emitters, size_t n_emit, const rb_surfel* d_surfels, const uint32_t* d_seeds,
                           size_t n, const rb_light_params* params, uint32_t first_sample, uint32_t samples, rb_radiance* d_out);

/* ---- Direct light with a weighted pick: emitters picked by power or by a caller's table of weights (the
 * normative definition; renderbaby_amd/direct.py: emitter_weights, emitter_cdf, pick_cdf, rays(cdf=...), bit for bit).  The
 * entry points above pick uniformly and are unchanged; these stand beside them.
 *   WEIGHT  of record j of N <= RB_MAX_EMITTERS: m = max(max(em.x, em.y), em.z), p = min(m * area, 3.4028235e38f) when the record
 *           is good in ITEM's sense (a, b, c, emissive, area finite, area > 0, a known kind), m > 0 and p > 0; else p = 0.
 *   TABLE   pmax = max p_j; L the smallest integer with 2^L >= N; S = 2^(24 - L);
 *           q_j = p_j > 0 ? max(1u, (uint32_t)((p_j / pmax) * (float)S)) : 0u; cdf[j] = q_0 + ... + q_j (uint32_t, inclusive);
 *           Q = cdf[N - 1] <= 2^24.  Integer sums: the table does not depend on the order of the scan that makes it.
 *   PICK    Q == 0 or Q > 2^24: no pick.  Else t = min((uint32_t)(u0 * (float)Q), Q - 1) and
 *           lo = 0, len = N; while (len > 1) { half = len >> 1; if (cdf[lo + half - 1] <= t) { lo += half; len -= half; } else
 *           len = half; } j = lo -- the first j with cdf[j] > t in a non-decreasing table, and inside [0, N - 1] for any
 *           contents; q = cdf[j] - (j ? cdf[j - 1] : 0), wrapping; q == 0: no pick.
 *   ITEM    section 21's with E = emitters[j] and g = ((((cs * ce) * area) / d2) * ((float)Q / (float)q)) * 0.318309886f.  An item
 *           without a pick is what an item of an empty table is: bound 0, colour +0, d = 0 0 0, valid if its surfel is.
 * cdf[j] = j + 1, and the table of equal powers, give rb_light_rays' bits. */
/* TABLE by power of n_emit records, host arrays, no engine, made on `device` (-1 = current): cdf_out[n_emit].  n_emit == 0 is
 * RB_OK; NULL emitters or cdf_out with n_emit > 0: RB_ERR_NULL_ARGUMENT; n_emit > RB_MAX_EMITTERS: RB_ERR_INVALID_OPTIONS. */
int rb_emitter_cdf(int32_t device, const rb_emitter* emitters, size_t n_emit, uint32_t* cdf_out);
/* TABLE by power of the engine's own emitter table, by rb_scene_emitters' protocol: min(*count, capacity) entries are written
 * (out may be NULL with capacity 0), *count is always the total.  Made on the device by the first call that needs it after
 * the emitter table and kept until the next rb_update; rb_last_query_ms reports the kernel time of that build (the emitter
 * table's own is not in it), 0 when the table stood.  rb_scene_emitters and rb_direct_light never make it. */
int rb_scene_emitter_cdf(rb_engine* e, uint32_t* out, size_t capacity, size_t* count);
/* The same into device memory of the engine's device: d_out and d_count 4-byte aligned; queued, as rb_scene_emitters_device. */
int rb_scene_emitter_cdf_device(rb_engine* e, uint32_t* d_out, size_t capacity, uint32_t* d_count);
/* rb_light_rays with PICK by cdf[n_emit]; cdf == NULL: by the TABLE by power of `emitters`, made for this call.  rb_light_rays'
 * refusals, and RB_ERR_INVALID_OPTIONS for a cdf that decreases somewhere or whose last entry is above 2^24. */
int rb_light_rays_cdf(int32_t device, const rb_emitter* emitters, const uint32_t* cdf, size_t n_emit, const rb_surfel* surfels,
                      const uint32_t* seeds, size_t n, const rb_light_params* params, uint32_t first_sample, uint32_t samples, rb_ray* rays_out,
                      float* tmax_out, float* contrib_out);
/* rb_direct_light with PICK by a table.  emitters == NULL: the scene's table with the scene's kept TABLE by power; cdf must be
 * NULL too, else RB_ERR_INVALID_OPTIONS.  emitters given and cdf == NULL: the TABLE by power of these records, made for this
 * call in the engine's scratch and queued -- nothing waits.  Both given: the caller's weights, n_emit of them; the host form
 * refuses a table that decreases somewhere or ends above 2^24 (RB_ERR_INVALID_OPTIONS) before a device is touched.  Everything
 * else -- refusals, side effects, pieces, sharded engines, multi-device handles, the reported names and times -- as
 * rb_direct_light; a refused call has done nothing. */
int rb_direct_light_cdf(rb_engine* e, const rb_emitter* emitters, const uint32_t* cdf, size_t n_emit, const rb_surfel* surfels,
                        const uint32_t* seeds, size_t n, const rb_light_params* params, uint32_t first_sample, uint32_t samples, rb_radiance* out);
/* The same on device memory of the engine's device; d_cdf (4-byte aligned, n_emit entries) is range-checked like every other
 * buffer but not read by the host: PICK defines the result for any contents, and every index it reads is inside the table. */
int rb_direct_light_cdf_device(rb_engine* e, const rb_emitter* d_emitters, const uint32_t* d_cdf, size_t n_emit, const rb_surfel* d_surfels,
                               const uint32_t* d_seeds, size_t n, const rb_light_params* params, uint32_t first_sample, uint32_t samples,
                               rb_radiance* d_out);

/* ---- Direct light with the emitters picked per grid cell (the normative definition;
 * renderbaby_amd/direct.py: emitter_bounds, grid_weights, emitter_grid_cdf, grid_cell, rays(grid=...), bit for bit).  Power
 * knows neither distance nor occlusion (section 23.5); here every cell of a regular grid has a table of its own, weighted by
 * power over squared distance, and an item searches the table of the cell its surfel lies in.  Additive: nothing above changes.
 * max(x, y) is `x > y ? x : y` and min(x, y) is `x < y ? x : y` throughout, so no weight is ever a NaN.
 *   GRID    an rb_probe_grid under rb_light_points' validation (finite origin, finite step > 0, counts >= 1, pad words and
 *           flags 0) whose counts count CELLS: cell (ix, iy, iz) spans origin + i step .. origin + (i + 1) step; rows =
 *           nx ny nz, row = (iz ny + iy) nx + ix.  tables is uint32_t[rows N]; row r is tables[r N .. r N + N - 1], one
 *           inclusive table in section 23's sense.  rows max(N, 1) > RB_MAX_GRID_ENTRIES: RB_ERR_INVALID_OPTIONS.
 *   BOUND   of record j (good, weighable and p_j are section 23's).  Triangle: ce = a + ((b + c) * 0.33333334f),
 *           re = sqrt(max(max(|a - ce|^2, |(a + b) - ce|^2), |(a + c) - ce|^2)), a squared length (x x + y y) + z z.
 *           Any other kind: ce = a, re = fabsf(b.x).
 *   WEIGHT  of record j in cell r: cc_a = origin_a + ((float)i_a + 0.5f) * step_a; hd = sqrt(0.25f * ((sx sx + sy sy) + sz sz));
 *           v = ce - cc, d2 = (v.x v.x + v.y v.y) + v.z v.z; r0 = re + hd, fl = r0 * r0;
 *           w = p_j > 0 ? min(p_j / max(d2, fl), 3.4028235e38f) : 0; wmax_r = max_j w; S = 2^(24 - L) as in section 23;
 *           q_j = p_j > 0 ? (wmax_r > 0 ? max(1u, (uint32_t)((w / wmax_r) * (float)S)) : 1u) : 0u; the row is the inclusive
 *           uint32_t sum of q, Q_r <= N S <= 2^24.  The floor of 1 goes with p_j > 0, not with w > 0: an emitter whose w
 *           underflows, or whose d2 overflows, stays reachable and the estimator keeps its mean for every grid.
 *   ITEM    section 23's in every line but the table it searches.  A valid surfel, per axis: f = (pos_a - origin_a) / step_a,
 *           i_a = min((uint32_t)max(f, 0.0f), count_a - 1), the conversion truncating and saturating; pos is the surfel's
 *           position as given, not the offset origin.  cdf = tables + row N; the pick, q, Q, the factor (float)Q / (float)q,
 *           "no pick" and all that follows are section 23's.  A point outside the grid takes the nearest cell.  For any
 *           contents of tables every index read lies in [0, rows N - 1].  An invalid surfel makes no pick; three draws always.
 * A grid whose every row is a table T gives rb_light_rays_cdf's bits with T (1 x 1 x 1 is the smallest case); rows of j + 1
 * give rb_light_rays' bits. */
#define RB_MAX_GRID_ENTRIES (1u << 26)
/* The tables of n_emit records over `grid`, host arrays, no engine, made on `device` (-1 = current): tables_out[rows n_emit].
 * Before a device is touched: NULL grid, or NULL emitters / tables_out with n_emit > 0: RB_ERR_NULL_ARGUMENT; n_emit >
 * RB_MAX_EMITTERS, a bad grid, the entry cap: RB_ERR_INVALID_OPTIONS.  n_emit == 0 is RB_OK. */
int rb_emitter_grid_cdf(int32_t device, const rb_emitter* emitters, size_t n_emit, const rb_probe_grid* grid, uint32_t* tables_out);
/* The same into device memory of the engine's device (d_tables_out 4-byte aligned, d_emitters 16-byte).  d_emitters == NULL:
 * the scene's kept emitter table; n_emit must then equal its count (rb_scene_emitters), else RB_ERR_INVALID_OPTIONS.  Queued
 * on the engine's stream, nothing waits once the emitter table stands.  The engine keeps no grid: the caller keeps
 * d_tables_out as long as it likes and passes it back.  rb_last_query_kernel_name reports "k_grid_rows", rb_last_query_ms the
 * build's kernel time (the emitter table's own is not in it). */
int rb_emitter_grid_cdf_device(rb_engine* e, const rb_emitter* d_emitters, size_t n_emit, const rb_probe_grid* grid, uint32_t* d_tables_out);
/* rb_light_rays with ITEM above; tables == NULL: made for this call.  rb_light_rays' refusals, the grid's, and
 * RB_ERR_INVALID_OPTIONS for a row of tables that decreases somewhere or ends above 2^24. */
int rb_light_rays_grid(int32_t device, const rb_emitter* emitters, const rb_probe_grid* grid, const uint32_t* tables, size_t n_emit,
                       const rb_surfel* surfels, const uint32_t* seeds, size_t n, const rb_light_params* params, uint32_t first_sample,
                       uint32_t samples, rb_ray* rays_out, float* tmax_out, float* contrib_out);
/* rb_direct_light with ITEM above.  emitters == NULL: the scene's table, and n_emit must equal its count.  tables == NULL:
 * made for this call in the engine's scratch and queued, nothing waits; tables given (with or without emitters): rows n_emit
 * entries, which the host form reads -- a row that decreases somewhere or ends above 2^24 is RB_ERR_INVALID_OPTIONS.  The
 * pieces of a call share one set of tables.  Every refusal of rb_direct_light, rb_light_points' of the grid, the entry cap
 * and a NULL grid (RB_ERR_NULL_ARGUMENT) come before a device is touched; a refused call has done nothing.  Side effects,
 * pieces, sharded engines, multi-device handles, the reported names and times as rb_direct_light_cdf. */
int rb_direct_light_grid(rb_engine* e, const rb_emitter* emitters, const rb_probe_grid* grid, const uint32_t* tables, size_t n_emit,
                         const rb_surfel* surfels, const uint32_t* seeds, size_t n, const rb_light_params* params, uint32_t first_sample,
                         uint32_t samples, rb_radiance* out);
/* The same on device memory of the engine's device; d_tables (4-byte aligned, rows n_emit entries) is range-checked like every
 * other buffer but not read by the host: ITEM defines the result for any contents. */
int rb_direct_light_grid_device(rb_engine* e, const rb_emitter* d_emitters, const rb_probe_grid* grid, const uint32_t* d_tables, size_t n_emit,
                                const rb_surfel* d_surfels, const uint32_t* d_seeds, size_t n, const rb_light_params* params,
                                uint32_t first_sample, uint32_t samples, rb_radiance* d_out);

/* ---- Per-cell tables that learn visibility from tallies (the normative definition;
 * renderbaby_amd/direct.py: tally, grid_weights(tally=...), emitter_grid_cdf(tally=...), bit for bit).  Section 24's weight has no
 * visibility term; every direct-light call pays for one -- the any-hit byte of every shadow ray -- and the fold forgets which
 * emitter in which cell it belonged to.  Here the caller keeps that answer and the table build uses it.  Additive: nothing
 * above changes.
 *   TALLY   rb_grid_tally[rows N], record r N + j belongs to emitter j in cell r (GRID of section 24, the same cap).  uint32_t
 *           sums that wrap; the caller owns the array, its lifetime and its zeroing.
 *   COUNT   item (i, k) of a grid call has section 24's row r and pick j.  It is counted when the bound stored for it is > 0:
 *           valid, picked and lit, a real shadow ray.  A counted item adds 1 to tried[r N + j], and 1 to seen[r N + j] if its
 *           result byte is RB_OCCL_VISIBLE.  Invalid surfels, items without a pick, items facing away and padding count nothing.
 *           Integer atomics: the sums are exact in any order.
 *   WEIGHT  t = tried, s = min(seen, tried), prior a finite with 0 < a <= 16777216: f = ((float)s + a) / ((float)t + a);
 *           w' = w * f with w of section 24; wmax_r, q_j and the row as section 24 with w' for w; the floor of 1 stays with
 *           p_j > 0.  f is in [0, 1] and never a NaN -- above 0 for a >= 2^-117, below that it can underflow --, and an emitter
 *           with power stays reachable by the floor, so the estimator keeps its mean for any tally.  An all-zero tally, and one
 *           with seen >= tried everywhere, give rb_emitter_grid_cdf's rows bit for bit (f = 1).
 * Tables are unbiased for any samples that did not go into their tally: train on one sample range, render another. */
typedef struct rb_grid_tally {
    uint32_t tried, seen;
} rb_grid_tally;
/* rb_direct_light_grid with one more argument, the tally (rows n_emit records), read and written: the count of every piece is
 * queued behind its walk and its kernel time is added to the call's.  out may be NULL for a training-only call (no fold runs);
 * with out given the sums are rb_direct_light_grid's bits.  The host form uploads the tally once, every piece adds to the one
 * device copy, and the call downloads it at the end.  tally == NULL: RB_ERR_NULL_ARGUMENT.  Every other refusal is
 * rb_direct_light_grid's, comes before a device is touched and leaves the tally unwritten.  Pieces, sharded engines,
 * multi-device handles, the reported names and times as rb_direct_light_grid. */
int rb_direct_light_grid_tally(rb_engine* e, const rb_emitter* emitters, const rb_probe_grid* grid, const uint32_t* tables, size_t n_emit,
                               const rb_surfel* surfels, const uint32_t* seeds, size_t n, const rb_light_params* params,
                               uint32_t first_sample, uint32_t samples, rb_radiance* out, rb_grid_tally* tally);
/* The same on device memory of the engine's device: d_tally (4-byte aligned, rows n_emit records) is range-checked, the call
 * queues and returns. */
int rb_direct_light_grid_tally_device(rb_engine* e, const rb_emitter* d_emitters, const rb_probe_grid* grid, const uint32_t* d_tables,
                                      size_t n_emit, const rb_surfel* d_surfels, const uint32_t* d_seeds, size_t n,
                                      const rb_light_params* params, uint32_t first_sample, uint32_t samples, rb_radiance* d_out,
                                      rb_grid_tally* d_tally);
/* rb_emitter_grid_cdf with WEIGHT above: protocol and refusals are its own; a prior that is not finite, <= 0 or > 16777216 is
 * RB_ERR_INVALID_OPTIONS, a NULL tally with n_emit > 0 RB_ERR_NULL_ARGUMENT. */
int rb_emitter_grid_learned(int32_t device, const rb_emitter* emitters, size_t n_emit, const rb_probe_grid* grid, const rb_grid_tally* tally,
                            float prior, uint32_t* tables_out);
/* rb_emitter_grid_cdf_device with WEIGHT above; d_tally 4-byte aligned, range-checked.  The engine keeps nothing.
 * rb_last_query_kernel_name reports "k_grid_rows_seen". */
int rb_emitter_grid_learned_device(rb_engine* e, const rb_emitter* d_emitters, size_t n_emit, const rb_probe_grid* grid,
                                   const rb_grid_tally* d_tally, float prior, uint32_t* d_tables_out);

/* ---- Edge-avoiding denoiser over the first-hit buffers (no reference counterpart).  An a-trous wavelet
 * filter (Dammertz et al. 2010) on the albedo-demodulated mean radiance, guided by the first hit of every pixel-centre ray.
 * Section 13 is the normative definition: every step one IEEE binary32 operation in a fixed order, so that the device's result
 * equals the numpy model renderbaby_amd/denoise.py bit for bit.  The one exception: a NaN the filter itself generates (0 * inf,
 * inf - inf, 0 / 0, inf / inf) has unspecified sign and payload; everything else, including which words are NaN, is as written.
 * All buffers are in the orientation of the delivered frame (row-major, top row first, x mirrored). */
typedef struct rb_guide {                                                                           /* 48 B */
    float normal[3];    /* the first hit's rb_hit.normal, unchanged */
    float t;            /* its rb_hit.t */
    float pos[3];       /* origin + t * d, one multiply and one add per component; d: the direction the query kernel normalised */
    uint32_t cls;       /* the hit's RB_HIT_* kind if the pixel is filterable; 0 = pass-through: NONE, INVALID, LIGHT, any emissive component > 0 */
    float albedo[3];    /* its rb_surface.albedo, unchanged */
    float _pad;
} rb_guide;
typedef struct rb_denoise_params {                                                                  /* 32 B */
    uint32_t iterations;         /* 0..8; iteration i taps at distance 2^i; 0: the mean radiance passes through, no demodulation */
    uint32_t normal_power_log2;  /* 0..10: max(0, n_p . n_q) is squared this many times */
    float sigma_depth;           /* > 0: plane distance |n_p . (P_q - P_p)| at which a tap's weight reaches 0, as a share of t_p */
    float sigma_color;           /* colour edge-stopping width of iteration 0 (halved per iteration); <= 0 switches the term off */
    float albedo_floor;          /* > 0: demodulation divides by max(albedo, albedo_floor) */
    uint32_t flags;              /* must be 0 */
    uint32_t _reserved[2];       /* must be 0 */
} rb_denoise_params;
/* The defaults (DESIGN.md section 13 records the measurements that chose them). */
int rb_denoise_default_params(rb_denoise_params* p);
/* The filter on its own, no engine: host arrays in and out, the work on `device` (-1 = current).  color4: the mean radiance,
 * w * h vec4 (the fourth component is ignored); guides: w * h records; out4 (w * h vec4, w = 1) and rgba_out (w * h RGBA8,
 * color_map(out / (out + 1))): either may be NULL, not both.  NULL params / color4 / guides: RB_ERR_NULL_ARGUMENT before any
 * device is touched; parameters out of range or non-finite, or w * h >= 2^31: RB_ERR_INVALID_OPTIONS; w * h == 0 is RB_OK. */
int rb_denoise_buffers(int32_t device, const rb_denoise_params* params, uint32_t w, uint32_t h, const float* color4,
                       const rb_guide* guides, float* out4, uint8_t* rgba_out);
/* The filter over the engine's committed accumulation (what rb_read_accumulation reads), guided by the engine's guide buffer:
 * made on the device by the first denoise after an accepted rb_update -- the pixel-centre rays through the query kernels of
 * the walk the scene takes, packed by one kernel -- and kept until the next accepted rb_update.  rgba_out (w * h * 4 bytes)
 * and linear_out (w * h vec4): either may be NULL, not both; page-locked destinations are recognised as by rb_render.  The
 * side effects are a query's: none on the accumulation, the frames, the colour buffer, rb_get_stats or the random sequence; a
 * pass the iterator has started ahead stays valid.  A sharded engine and a multi-device handle are RB_ERR_INVALID_OPTIONS (a
 * tap would cross a stripe boundary); before the first update: RB_ERR_NOT_INITIALIZED. */
int rb_denoise(rb_engine* e, const rb_denoise_params* params, uint8_t* rgba_out, float* linear_out);
/* The same with the outputs in device memory of the engine's device (validated like rb_cast_rays_device's buffers: a host
 * pointer, another device's memory, a misaligned pointer -- 4 bytes for d_rgba_out, 16 for d_linear_out -- or an allocation
 * that ends early is RB_ERR_INVALID_OPTIONS).  Queued on the engine's stream; returns without waiting: rb_sync is the wait. */
int rb_denoise_device(rb_engine* e, const rb_denoise_params* params, uint8_t* d_rgba_out, float* d_linear_out);
/* The guide buffer the engine filters with (w * h records; made now if the engine has none since its last update). */
int rb_denoise_guides(rb_engine* e, rb_guide* guides_out);
/* Measurement aid for tools/denoise_rate.py (it may change or go): kernel time of the most recent denoise -- prepare, iterations
 * and finish, HIP events on the engine's stream, ms -- and, if not NULL, of the guide build it had to make (0: it had the guides). */
int rb_last_denoise_ms(rb_engine* e, float* ms, float* guide_build_ms);

/* ---- Temporal reprojection: the previous frame's history carried across a camera move (the normative
 * definition; no reference counterpart).  The history half of a real-time path-tracing denoiser (Schied et al. 2017): every
 * pixel's first hit is projected into the previous camera, the previous frame's colour and sample count are taken along where
 * it saw the same surface there, and the current accumulation is merged onto them.  No variance, no filter: rb_denoise's
 * bits stay as they are.  Every step is one IEEE binary32 operation in the order section 22.1 fixes -- max / min are
 * `a > b ? a : b` / `a < b ? a : b` --, so the device equals the numpy model renderbaby_amd/temporal.py bit for bit, with
 * section 13's one exception for the sign and payload of a NaN the arithmetic itself generates.  All buffers are in the
 * orientation of the delivered frame (row-major, top row first, x mirrored), as rb_guide buffers and rb_denoise_buffers.
 * A frame record is a float[4]: {mean r, g, b, count}; count: the samples the mean stands for.  Its output feeds the next call
 * as prev4 and rb_denoise_buffers as color4.
 * REPROJECT, pixel p at displayed column Xp, row Yp; G = cur_guides[p], V the previous view, NONE = four +0.0f, a dot is
 * (x x + y y) + z z:  G.cls == 0 -> NONE.  e = G.pos - V.pos, z = e . V.fwd, a = e . V.right, b = e . V.up; !(z > 0) -> NONE.
 * X = V.cx - (a / z) * V.sx, Y = V.cy - (b / z) * V.sy; !(X > -1 && X < (float)w && Y > -1 && Y < (float)h) -> NONE.
 * X0 = floorf(X), fx = X - X0, ix = (int)X0 (the same for Y).  m_p[k] = max(G.albedo[k], albedo_floor), den = sigma_depth * G.t.
 * Taps dy = 0, 1 (outer), dx = 0, 1 (inner), q = (ix + dx, iy + dy), bw = (dx ? fx : 1 - fx) * (dy ? fy : 1 - fy); a tap is
 * skipped when q is outside the frame, !(bw > 0), prev_guides[q].cls != G.cls, a word of prev4[q] is non-finite or
 * !(prev4[q].count > 0), !(G.normal . Gq.normal >= normal_min), !(|G.normal . (Gq.pos - G.pos)| <= den).  An accepted tap:
 * hs[k] += bw * (prev4[q][k] / max(Gq.albedo[k], albedo_floor)), hn += bw * prev4[q].count, bs += bw.  !(bs > 0) -> NONE.
 * hist[k] = (hs[k] / bs) * m_p[k], hl = min(hn / bs, max_history); a non-finite word -> NONE, else {hist, hl}.
 * MERGE of hst (REPROJECT's result) and cur4[p] = {c, n}: out = cur4[p], the bits, if G.cls == 0, a word of cur4[p] is
 * non-finite, !(n >= 0) or hst.count == 0; else tot = hst.count + n, out[k] = (hst[k] * hst.count + c[k] * n) / tot, out.count = tot. */
typedef struct rb_view {            /* 64 B: a render camera as the inverse of the pixel-centre ray needs it */
    float pos[3];   float cx;       /* cx = wm1 * 0.5f */
    float right[3]; float cy;       /* cy = hm1 * 0.5f */
    float up[3];    float sx;       /* sx = cx / (fov * aspect) */
    float fwd[3];   float sy;       /* sy = cy / fov */
} rb_view;
typedef struct rb_reproject_params {   /* 32 B */
    float sigma_depth;    /* finite, > 0: a tap is the same surface if |n_p . (P_q - P_p)| <= sigma_depth * t_p  (section 13's plane distance) */
    float normal_min;     /* finite, -1 .. 1: ... and n_p . n_q >= normal_min */
    float albedo_floor;   /* finite, > 0: section 13's demodulation floor */
    float max_history;    /* finite, >= 1: cap of the carried sample count */
    uint32_t flags;       /* must be 0 */
    uint32_t _reserved[3];/* must be 0 */
} rb_reproject_params;
/* The view of a render camera at w x h: aspect, fwd, right, up, fov, wm1 and hm1 by the steps of a render launch, in its order,
 * then the four scalars as the comments above state, one operation each.  Host only: no device is touched.  NULL: RB_ERR_NULL_ARGUMENT. */
int rb_view_from_camera(const rb_camera* cam, uint32_t w, uint32_t h, rb_view* out);
/* sigma_depth 0.02 and albedo_floor 0.01 (the denoiser's), normal_min 0.9 and max_history 32. */
int rb_reproject_default_params(rb_reproject_params* p);
/* REPROJECT, and with cur4 MERGE on top, no engine: host arrays of w * h records in and out, the work on `device` (-1 =
 * current).  cur4 == NULL: REPROJECT alone.  Before any device is touched: NULL params / prev_view / prev4 / prev_guides /
 * cur_guides / out4: RB_ERR_NULL_ARGUMENT; a parameter out of range or non-finite, a non-finite word in the view, non-zero
 * flags or reserved words, w * h >= 2^31: RB_ERR_INVALID_OPTIONS; w * h == 0 is RB_OK. */
int rb_reproject_buffers(int32_t device, const rb_reproject_params* params, uint32_t w, uint32_t h, const rb_view* prev_view,
                         const float* prev4, const rb_guide* prev_guides, const rb_guide* cur_guides, const float* cur4, float* out4);
/* The same with every buffer in device memory of the engine's device, 16-byte aligned, validated as rb_cast_rays_device's;
 * d_cur4 may be NULL.  The engine lends its device and its stream, as to rb_light_points_device: queued there, not waited for
 * (rb_sync is the wait); RB_ERR_NOT_INITIALIZED before the first update; a multi-device handle answers on devices[0];
 * rb_last_query_kernel_name reports "k_reproject", rb_last_query_ms its time. */
int rb_reproject_device(rb_engine* e, const rb_reproject_params* params, uint32_t w, uint32_t h, const rb_view* prev_view,
                        const float* d_prev4, const rb_guide* d_prev_guides, const rb_guide* d_cur_guides, const float* d_cur4, float* d_out4);
/* What a viewer calls once per displayed frame, after its passes.  The engine keeps a history H (a frame-record plane, a copy
 * of the guide planes, their rb_view and size, a valid flag) and a base B (one frame-record plane, valid until the next
 * accepted rb_update).  A call: the guides (as rb_denoise); if B is not valid, B = REPROJECT(H -> the current guides) -- every
 * record NONE if H is invalid, of another size or has a non-finite view --; F = MERGE(B, {the mean radiance of section 13.1,
 * acc.w}); H = {F, the current guide planes, the current view}; rb_denoise's filter on F with dparams into the outputs.
 * B keeps repeated calls within one update from counting their own samples twice.  rparams / dparams NULL:
 * RB_ERR_NULL_ARGUMENT.  Outputs, side effects and refusals are rb_denoise's; a refused call changes nothing, H included;
 * with no valid history the outputs are rb_denoise's bit for bit. */
int rb_denoise_history(rb_engine* e, const rb_reproject_params* rparams, const rb_denoise_params* dparams, uint8_t* rgba_out,
                       float* linear_out);
/* ... with the outputs in device memory, as rb_denoise_device. */
int rb_denoise_history_device(rb_engine* e, const rb_reproject_params* rparams, const rb_denoise_params* dparams, uint8_t* d_rgba_out,
                              float* d_linear_out);
/* F of the most recent rb_denoise_history (w * h frame records), for tests and tools; no history, or one of another
 * size than the current frame: RB_ERR_NOT_INITIALIZED. */
int rb_history_read(rb_engine* e, float* out4);
/* Drops H and B: the next rb_denoise_history starts without history. */
int rb_history_reset(rb_engine* e);
/* Measurement aid for tools/reproject_rate.py (it may change or go): kernel time of REPROJECT (0: the base was valid) plus MERGE
 * in the most recent rb_denoise_history, HIP events on the engine's stream, ms. */
int rb_last_reproject_ms(rb_engine* e, float* ms);

/* Which builder produced the library's own tree: "host-sah", "device-ploc", "device-lbvh", or "" when
 * there is none (flag not set, single-node tree, or the scene keeps the exact walk).  Valid after the
 * first rb_dispatch / rb_render that follows an update.  `build_ms`, if not NULL, receives the wall
 * time of that build including its uploads. */
const char* rb_fast_bvh_builder(const rb_engine* e, float* build_ms);

/* Which builder produced the library's sphere tree (scenes with more than 64 spheres): "device-median", "host-median", or
 * "" when the engine scans (<= 64 spheres, RB_FLAG_NO_SPHERE_BVH).  Valid after the rb_update that brought the spheres.
 * `build_ms`, if not NULL, receives the wall time of that build including its uploads. */
const char* rb_sphere_tree_builder(const rb_engine* e, float* build_ms);

/* Library / device identification for logs. */
const char* rb_version(void);
int rb_device_name(int device, char* buf, size_t buf_len);

#ifdef __cplusplus
} /* extern "C" */

static_assert(sizeof(rb_camera) == 48, "Camera is 48 B");
static_assert(sizeof(rb_uniforms) == 144, "Uniforms is 144 B");
static_assert(sizeof(rb_material) == 80, "Material is 80 B");
static_assert(sizeof(rb_sphere) == 96, "Sphere is 96 B");
static_assert(sizeof(rb_point_light) == 96, "PointLight is 96 B");
static_assert(sizeof(rb_mesh) == 96, "Mesh is 96 B");
static_assert(sizeof(rb_bvh_node) == 48, "BVHNode is 48 B");
static_assert(sizeof(rb_gpu_triangle) == 64, "GPUTriangle is 64 B");
static_assert(sizeof(rb_texture_info) == 16, "TextureInfo is 16 B");
static_assert(sizeof(rb_progressive) == 16, "ProgressiveRenderHelper is 16 B");
static_assert(offsetof(rb_uniforms, camera) == 16, "camera @16");
static_assert(offsetof(rb_uniforms, spheres_count) == 64, "spheres_count @64");
static_assert(offsetof(rb_uniforms, ground_height) == 84, "ground_height @84");
static_assert(offsetof(rb_uniforms, sky_color) == 96, "sky_color @96");
static_assert(offsetof(rb_uniforms, max_depth) == 108, "max_depth @108");
static_assert(offsetof(rb_uniforms, checkerboard_color_1) == 112, "cb1 @112");
static_assert(offsetof(rb_uniforms, checkerboard_color_2) == 128, "cb2 @128");
static_assert(offsetof(rb_camera, pos) == 16, "pos @16");
static_assert(offsetof(rb_camera, dir) == 32, "dir @32");
static_assert(offsetof(rb_material, diffuse) == 16, "diffuse @16");
static_assert(offsetof(rb_material, specular) == 32, "specular @32");
static_assert(offsetof(rb_material, shininess) == 44, "shininess @44");
static_assert(offsetof(rb_material, emissive) == 48, "emissive @48");
static_assert(offsetof(rb_material, texture_index) == 72, "texture_index @72");
static_assert(offsetof(rb_bvh_node, left) == 32, "left @32");
static_assert(offsetof(rb_gpu_triangle, mesh_index) == 48, "mesh_index @48");
static_assert(sizeof(rb_ray) == 32, "rb_ray is 32 B");
static_assert(sizeof(rb_hit) == 48, "rb_hit is 48 B");
static_assert(sizeof(rb_surface) == 48, "rb_surface is 48 B");
static_assert(offsetof(rb_ray, dir) == 16, "dir @16");
static_assert(offsetof(rb_hit, u) == 16, "u @16");
static_assert(offsetof(rb_hit, normal) == 32, "normal @32");
static_assert(offsetof(rb_surface, flags) == 12, "flags @12");
static_assert(offsetof(rb_surface, emissive) == 16, "emissive @16");
static_assert(offsetof(rb_surface, texture_index) == 28, "texture_index @28");
static_assert(offsetof(rb_surface, uv) == 32, "uv @32");
static_assert(sizeof(rb_radiance) == 16, "rb_radiance is 16 B");
static_assert(sizeof(rb_camera_ex) == 96, "rb_camera_ex is 96 B");
static_assert(offsetof(rb_camera_ex, pos) == 16, "pos @16");
static_assert(offsetof(rb_camera_ex, forward) == 64, "forward @64");
static_assert(offsetof(rb_camera_ex, focus_distance) == 80, "focus_distance @80");
static_assert(sizeof(rb_surfel) == 32, "rb_surfel is 32 B");
static_assert(offsetof(rb_surfel, normal) == 16, "normal @16");
static_assert(sizeof(rb_hemi_params) == 32, "rb_hemi_params is 32 B");
static_assert(sizeof(rb_openness) == 8, "rb_openness is 8 B");
static_assert(sizeof(rb_lightmap_params) == 32, "rb_lightmap_params is 32 B");
static_assert(offsetof(rb_lightmap_params, offset) == 16, "offset @16");
static_assert(sizeof(rb_probe) == 16, "rb_probe is 16 B");
static_assert(sizeof(rb_sh9) == 112, "rb_sh9 is 112 B");
static_assert(offsetof(rb_sh9, weight) == 108, "weight @108");
static_assert(sizeof(rb_probe_grid) == 48, "rb_probe_grid is 48 B");
static_assert(offsetof(rb_probe_grid, step) == 16, "step @16");
static_assert(offsetof(rb_probe_grid, counts) == 32, "counts @32");
static_assert(offsetof(rb_probe_grid, flags) == 44, "flags @44");
static_assert(sizeof(rb_lit) == 16, "rb_lit is 16 B");
static_assert(sizeof(rb_probe_depth) == 1024, "rb_probe_depth is 1024 B");
static_assert(sizeof(rb_light_visibility) == 16, "rb_light_visibility is 16 B");
static_assert(offsetof(rb_light_visibility, flags) == 8, "flags @8");
static_assert(sizeof(rb_emitter) == 64, "rb_emitter is 64 B");
static_assert(offsetof(rb_emitter, b) == 16, "b @16");
static_assert(offsetof(rb_emitter, area) == 44, "area @44");
static_assert(offsetof(rb_emitter, emissive) == 48, "emissive @48");
static_assert(sizeof(rb_light_params) == 32, "rb_light_params is 32 B");
static_assert(sizeof(rb_grid_tally) == 8, "rb_grid_tally is 8 B");
static_assert(offsetof(rb_light_params, mask) == 8, "mask @8");
static_assert(sizeof(rb_guide) == 48, "rb_guide is 48 B");
static_assert(sizeof(rb_denoise_params) == 32, "rb_denoise_params is 32 B");
static_assert(offsetof(rb_guide, t) == 12, "t @12");
static_assert(offsetof(rb_guide, pos) == 16, "pos @16");
static_assert(offsetof(rb_guide, cls) == 28, "cls @28");
static_assert(offsetof(rb_guide, albedo) == 32, "albedo @32");
static_assert(offsetof(rb_denoise_params, sigma_depth) == 8, "sigma_depth @8");
static_assert(offsetof(rb_denoise_params, flags) == 20, "flags @20");
static_assert(sizeof(rb_view) == 64, "rb_view is 64 B");
static_assert(offsetof(rb_view, cx) == 12, "cx @12");
static_assert(offsetof(rb_view, right) == 16, "right @16");
static_assert(offsetof(rb_view, up) == 32, "up @32");
static_assert(offsetof(rb_view, fwd) == 48, "fwd @48");
static_assert(offsetof(rb_view, sy) == 60, "sy @60");
static_assert(sizeof(rb_reproject_params) == 32, "rb_reproject_params is 32 B");
static_assert(offsetof(rb_reproject_params, max_history) == 12, "max_history @12");
static_assert(offsetof(rb_reproject_params, flags) == 16, "flags @16");
#else
_Static_assert(sizeof(rb_camera) == 48, "Camera is 48 B");
_Static_assert(sizeof(rb_uniforms) == 144, "Uniforms is 144 B");
_Static_assert(sizeof(rb_material) == 80, "Material is 80 B");
_Static_assert(sizeof(rb_sphere) == 96, "Sphere is 96 B");
_Static_assert(sizeof(rb_point_light) == 96, "PointLight is 96 B");
_Static_assert(sizeof(rb_mesh) == 96, "Mesh is 96 B");
_Static_assert(sizeof(rb_bvh_node) == 48, "BVHNode is 48 B");
_Static_assert(sizeof(rb_gpu_triangle) == 64, "GPUTriangle is 64 B");
_Static_assert(sizeof(rb_texture_info) == 16, "TextureInfo is 16 B");
_Static_assert(sizeof(rb_progressive) == 16, "ProgressiveRenderHelper is 16 B");
_Static_assert(sizeof(rb_ray) == 32, "rb_ray is 32 B");
_Static_assert(sizeof(rb_hit) == 48, "rb_hit is 48 B");
_Static_assert(sizeof(rb_surface) == 48, "rb_surface is 48 B");
_Static_assert(sizeof(rb_radiance) == 16, "rb_radiance is 16 B");
_Static_assert(sizeof(rb_camera_ex) == 96, "rb_camera_ex is 96 B");
_Static_assert(sizeof(rb_surfel) == 32, "rb_surfel is 32 B");
_Static_assert(sizeof(rb_hemi_params) == 32, "rb_hemi_params is 32 B");
_Static_assert(sizeof(rb_openness) == 8, "rb_openness is 8 B");
_Static_assert(sizeof(rb_lightmap_params) == 32, "rb_lightmap_params is 32 B");
_Static_assert(sizeof(rb_probe) == 16, "rb_probe is 16 B");
_Static_assert(sizeof(rb_sh9) == 112, "rb_sh9 is 112 B");
_Static_assert(sizeof(rb_probe_grid) == 48, "rb_probe_grid is 48 B");
_Static_assert(sizeof(rb_lit) == 16, "rb_lit is 16 B");
_Static_assert(sizeof(rb_probe_depth) == 1024, "rb_probe_depth is 1024 B");
_Static_assert(sizeof(rb_light_visibility) == 16, "rb_light_visibility is 16 B");
_Static_assert(sizeof(rb_emitter) == 64, "rb_emitter is 64 B");
_Static_assert(sizeof(rb_light_params) == 32, "rb_light_params is 32 B");
_Static_assert(sizeof(rb_grid_tally) == 8, "rb_grid_tally is 8 B");
_Static_assert(sizeof(rb_guide) == 48, "rb_guide is 48 B");
_Static_assert(sizeof(rb_denoise_params) == 32, "rb_denoise_params is 32 B");
_Static_assert(sizeof(rb_view) == 64, "rb_view is 64 B");
_Static_assert(sizeof(rb_reproject_params) == 32, "rb_reproject_params is 32 B");
#endif

#endif /* RB_ABI_H */
