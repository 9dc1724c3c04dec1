// rb_queries.cpp -- what an engine answers besides frames: closest-hit queries (rb_cast_rays / rb_render_hits / rb_pick), any-hit
// occlusion, path-traced radiance along given rays, camera and hemisphere rays, lightmap texels and irradiance probes made on the
// device, light points from a baked probe grid with or without the probes' depth moments, direct light by shadow rays to the
// scene's emitters picked uniformly or by a table of weights, with their device forms, their getters and their C entry points
// (rb_abi.h; DESIGN.md sections 11-23; the
// denoiser and the frame's history: rb_frame.cpp).
// Every sequence is here once: one prologue (query_prologue), one timed
// launch (timed_launch), one runner per form -- run_pieces for the host forms, device_query_locked for the device forms --, over
// them one runner for the families of "n items, `samples` each" in both forms (run_family: radiance, camera, hemisphere,
// probes), one shape for the engine entry points (engine_entry) and one scope for the engine-less forms (DeviceScope).  The
// engine's state is rb_engine.hpp's; the launchers are rb_internal.hpp's; what rb_frame.cpp needs too is rb_queries.hpp's.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "rb_queries.hpp"

namespace {

using rb::copy_error, rb::device_range, rb::DeviceScope, rb::ensure_prepared, rb::frame_piece_rows, rb::page_locked, rb::query_copy_out,
    rb::reproject_check, rb::require_ready, rb::scene_params, rb::stage_ms;

// ------------------------------------------------------------------ closest-hit queries ----
// (rb_abi.h)  A query reads the scene and writes its own scratch: it is queued on the engine's stream
// behind whatever runs there -- a pass the iterator has started ahead included, which stays valid -- and uses events of its
// own, so neither the work counters nor the timing of a launch group move.

// what every query begins with; the kernel times of the query before -- rb_last_query_ms and those of its generator and
// projection stages -- are gone from here on, however far this one gets.  p == nullptr: a query that reads no scene
// (section 19) -- nothing is prepared for it.
int query_prologue(rb_engine* e, rb::KParams* p) {
    for (rb::StageTimer* t : {&e->t_query, &e->t_generator, &e->t_sh, &e->t_depth}) t->reset();
    int rc = require_ready(e);
    if (!rc && p) rc = ensure_prepared(e);
    if (!rc && p) rc = scene_params(e, p);
    return rc;
}

// what both runners time: `launch(li)` queues a query's kernels as one pair of e->t_query and returns a HIP status
template <class Launch>
int timed_launch(rb_engine* e, const char* kind, Launch&& launch) {
    rb::LaunchInfo li{};
    HIP_TRY(e, e->t_query.begin(e->stream));
    const int st = launch(&li);
    if (st) return rb::fail(e, RB_ERR_DEVICE, "%s kernel launch failed: %s", kind, hipGetErrorString(static_cast<hipError_t>(st)));
    HIP_TRY(e, e->t_query.end(e->stream));
    if (li.kernel_name) e->last_query_kernel_name = li.kernel_name;
    return RB_OK;
}

// One array of a host form: item i of the call lies at host + i * stride in the caller's memory, item i of a piece at
// dev + i * stride in the scratch.  host == nullptr: the caller left this array out.
struct PieceIn { const void* host; void* dev; size_t stride; };
struct PieceOut { void* host; const void* dev; size_t stride; bool pinned; };   // pinned: host is page-locked (the runner finds out)

// The host forms' runner: n items in pieces of `piece`.  A piece's inputs are uploaded ahead of the events (the time between them
// stays the kernels'), `launch(done, m, li)` queues the kernels of items [done, done + m) over the scratch and returns a HIP
// status, the results are copied out behind them and waited for.  `kind` names the family where a launch fails.
template <size_t N, class Launch>
int run_pieces(rb_engine* e, const char* kind, size_t piece, size_t n, std::initializer_list<PieceIn> ins, PieceOut (&&outs)[N],
               Launch&& launch) {
    if (n == 0) return RB_OK;
    for (PieceOut& o : outs) o.pinned = page_locked(o.host);
    for (size_t done = 0; done < n; done += piece) {
        const size_t m = std::min(piece, n - done);
        // (from pageable memory the runtime stages the copy and returns when the source may be reused)
        for (const PieceIn& in : ins)
            if (in.host) HIP_TRY(e, hipMemcpyAsync(in.dev, static_cast<const char*>(in.host) + done * in.stride, m * in.stride, hipMemcpyHostToDevice, e->stream));
        int rc = timed_launch(e, kind, [&](rb::LaunchInfo* li) { return launch(done, m, li); });
        for (const PieceOut& o : outs)
            if (!rc && o.host) rc = query_copy_out(e, static_cast<char*>(o.host) + done * o.stride, o.dev, m * o.stride, o.pinned);
        if (rc) return rc;
        HIP_TRY(e, hipStreamSynchronize(e->stream));   // the scratch is the next piece's
        float ms = 0.0f;
        HIP_TRY(e, e->t_query.read(&ms));   // folded here: the next piece records the same pair again
    }
    return RB_OK;
}

// the device forms' runner: one timed launch on the caller's buffers; nothing is waited for
template <class Launch>
int device_query_locked(rb_engine* e, Launch&& launch) {
    rb::KParams p{};
    int rc = query_prologue(e, &p);
    if (!rc) rc = timed_launch(e, "query", [&](rb::LaunchInfo* li) { return launch(p, li); });
    return rc;   // rb_last_query_ms reads the pair when it is asked
}

// ... of a query that reads no scene: the engine lends its device and its stream; `launch(li)` returns a HIP status
template <class Launch>
int device_stream_locked(rb_engine* e, Launch&& launch) {
    const int rc = query_prologue(e, nullptr);
    return rc ? rc : timed_launch(e, "query", launch);
}

int cast_rays_locked(rb_engine* e, const rb_ray* rays, size_t n, rb_hit* hits_out, rb_surface* surf_out) {
    rb::KParams p{};
    const size_t piece = std::min<size_t>(n, rb::kQueryPiece);
    const int rc = query_prologue(e, &p);
    if (rc) return rc;
    HIP_TRY(e, e->q_rays.reserve(piece));
    HIP_TRY(e, e->q_hits.reserve(piece));
    if (surf_out) HIP_TRY(e, e->q_surf.reserve(piece));
    return run_pieces(e, "query", piece, n, {{rays, e->q_rays.ptr, sizeof(rb_ray)}},
                      {{hits_out, e->q_hits.ptr, sizeof(rb_hit)}, {surf_out, e->q_surf.ptr, sizeof(rb_surface)}},
                      [&](size_t, size_t m, rb::LaunchInfo* li) {
                          rb::QueryArgs q{};
                          q.rays = e->q_rays.ptr;
                          q.n = static_cast<uint32_t>(m);
                          q.hits = e->q_hits.ptr;
                          q.surf = surf_out ? e->q_surf.ptr : nullptr;
                          return rb::launch_query(p, q, e->stream, li);
                      });
}

// the pixel centres of rows [0, rows) x the whole width (global = image rows, else this shard's local rows), or of one pixel:
// rows * w items, of which piece `done` begins at row done / w
int pixel_hits_locked(rb_engine* e, uint32_t x0, uint32_t y0, uint32_t w, uint32_t rows, bool global, rb_hit* hits_out, rb_surface* surf_out) {
    rb::KParams p{};
    const uint32_t piece_rows = frame_piece_rows(w);
    const int rc = query_prologue(e, &p);
    if (rc) return rc;
    HIP_TRY(e, e->q_hits.reserve(static_cast<size_t>(std::min(piece_rows, rows)) * w));
    if (surf_out) HIP_TRY(e, e->q_surf.reserve(static_cast<size_t>(std::min(piece_rows, rows)) * w));
    return run_pieces(e, "query", static_cast<size_t>(piece_rows) * w, static_cast<size_t>(rows) * w, {},
                      {{hits_out, e->q_hits.ptr, sizeof(rb_hit)}, {surf_out, e->q_surf.ptr, sizeof(rb_surface)}},
                      [&](size_t done, size_t m, rb::LaunchInfo* li) {
                          rb::QueryArgs q{};
                          q.win_x = x0;
                          q.win_y = y0 + static_cast<uint32_t>(done / w);
                          q.win_w = w;
                          q.win_h = static_cast<uint32_t>(m / w);
                          q.win_global = global ? 1u : 0u;
                          q.hits = e->q_hits.ptr;
                          q.surf = surf_out ? e->q_surf.ptr : nullptr;
                          return rb::launch_query(p, q, e->stream, li);
                      });
}

// ---- any-hit occlusion and the device forms (rb_abi.h)
int occluded_locked(rb_engine* e, const rb_ray* rays, const float* tmax, size_t n, uint32_t mask, uint8_t* out) {
    rb::KParams p{};
    const int rc = query_prologue(e, &p);
    if (rc || n == 0) return rc;
    const size_t piece = std::min<size_t>(n, rb::kQueryPiece);
    HIP_TRY(e, e->q_rays.reserve(piece));
    if (tmax) HIP_TRY(e, e->q_tmax.reserve(piece));
    HIP_TRY(e, e->q_occl.reserve(piece));
    return run_pieces(e, "occlusion", piece, n, {{rays, e->q_rays.ptr, sizeof(rb_ray)}, {tmax, e->q_tmax.ptr, sizeof(float)}},
                      {{out, e->q_occl.ptr, 1}}, [&](size_t, size_t m, rb::LaunchInfo* li) {
                          rb::OcclArgs a{};
                          a.q.rays = e->q_rays.ptr;
                          a.q.n = static_cast<uint32_t>(m);
                          a.tmax = tmax ? e->q_tmax.ptr : nullptr;
                          a.out = e->q_occl.ptr;
                          a.mask = mask;
                          return rb::launch_occluded(p, a, e->stream, li);
                      });
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
// rays or pixels per piece of at most `limit` (ray or pixel, sample) items: whole blocks of 64, never a part of one's samples
// (samples <= 65536: at least one block)
size_t radiance_piece(size_t limit, uint32_t samples) { return std::max<size_t>((limit / samples) & ~size_t(63), 64); }
size_t piece_items(size_t limit, size_t n, uint32_t samples) { return std::min(n, radiance_piece(limit, samples)); }

// the scratch of one piece: a colour per item and the queue word; `records`: a ray record per item too (rays made on the device)
int radiance_scratch(rb_engine* e, size_t piece, uint32_t samples, bool records) {
    const size_t items = ((piece + 63) / 64) * 64 * samples;
    if (records) HIP_TRY(e, e->q_rays.reserve(items));
    HIP_TRY(e, e->rad_colors.reserve(items * 4));
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

// `each(done, m)` for every piece [done, done + m) of n items; it returns a HIP status, and the first bad one ends the loop
template <class Each>
int for_pieces(size_t n, size_t piece, Each&& each) {
    for (size_t done = 0; done < n; done += piece)
        if (const int st = each(done, std::min(piece, n - done))) return st;
    return 0;
}

// One array of a family's call, item i at caller + i * stride: host memory in the host form, where a piece of it goes through
// the engine's staging buffer `stage`, device memory in the device form, where device_range asks for `align` under `name`.
// caller == nullptr: the caller left this array out.
struct FamilyArray {
    const void* caller;
    size_t stride, align;
    const char* name;
    const char* stage_name;                               // the buffer as a failed reservation names it
    void* stage;
    hipError_t (*reserve)(void* stage, size_t n, void** ptr);   // room for n items in `stage`; *ptr: where they begin
};
template <class T>
FamilyArray family_array(const void* caller, rb::DevBuf<T>& stage, const char* stage_name, size_t align, const char* name) {
    return {caller, sizeof(T), align, name, stage_name, &stage, [](void* b, size_t n, void** ptr) {
                rb::DevBuf<T>* const buf = static_cast<rb::DevBuf<T>*>(b);
                const hipError_t st = buf->reserve(n);
                *ptr = buf->ptr;
                return st;
            }};
}
#define FAMILY_ARRAY(caller, stage, align, name) family_array(caller, stage, #stage, align, name)

// The runner of the families of "n > 0 items, `samples` samples each": pieces of whole blocks of 64 items and at most `limit`
// (item, sample) pairs.  `ins`: up to two input arrays, `out`: the result array.  `scratch(piece)` reserves what a piece needs
// beside them and returns an rb code; `piece_fn(p, in, out, done, m, li)` queues items [done, done + m) of the call, whose
// arrays begin at in[0], in[1] (nullptr: left out) and out (nullptr: the caller left the result out) in device memory, and
// returns a HIP status.
// Device form: the caller's buffers are checked, then every piece is queued on them between the query's two events (the pieces
// share the scratch in stream order); nothing is waited for.  Host form: run_pieces over the staging buffers.
template <class Scratch, class Piece>
int run_family(rb_engine* e, bool device, const char* kind, size_t limit, size_t n, uint32_t samples, const FamilyArray (&ins)[2],
               const FamilyArray& out, Scratch&& scratch, Piece&& piece_fn) {
    const size_t piece = piece_items(limit, n, samples);
    const void* in[2] = {nullptr, nullptr};
    if (device) {
        for (const FamilyArray& a : ins)
            if (a.caller)
                if (const int rc = device_range(e, a.caller, n * a.stride, a.align, a.name)) return rc;
        if (out.caller)   // (left out: a family that allows it has said so before it came here)
            if (const int rc = device_range(e, out.caller, n * out.stride, out.align, out.name)) return rc;
        return device_query_locked(e, [&](const rb::KParams& p, rb::LaunchInfo* li) {
            if (scratch(piece)) return static_cast<int>(hipErrorOutOfMemory);
            return for_pieces(n, piece, [&](size_t done, size_t m) {
                for (int k = 0; k < 2; k++) in[k] = ins[k].caller ? static_cast<const char*>(ins[k].caller) + done * ins[k].stride : nullptr;
                return piece_fn(p, in, out.caller ? static_cast<char*>(const_cast<void*>(out.caller)) + done * out.stride : nullptr, done, m, li);
            });
        });
    }
    rb::KParams p{};
    int rc = query_prologue(e, &p);
    if (!rc) rc = scratch(piece);
    if (rc) return rc;
    PieceIn staged[2] = {};
    void* d_out = nullptr;
    const auto reserve = [&](const FamilyArray& a, void** ptr) {
        const hipError_t st = a.reserve(a.stage, piece, ptr);
        return st == hipSuccess ? RB_OK : rb::fail(e, RB_ERR_DEVICE, "%s.reserve(piece) failed: %s", a.stage_name, hipGetErrorString(st));
    };
    for (int k = 0; k < 2; k++) {
        if (!ins[k].caller) continue;
        void* ptr = nullptr;
        if ((rc = reserve(ins[k], &ptr)) != RB_OK) return rc;
        staged[k] = PieceIn{ins[k].caller, ptr, ins[k].stride};
        in[k] = ptr;
    }
    if (out.caller && (rc = reserve(out, &d_out)) != RB_OK) return rc;
    return run_pieces(e, kind, piece, n, {staged[0], staged[1]}, {{const_cast<void*>(out.caller), d_out, out.stride}},
                      [&](size_t done, size_t m, rb::LaunchInfo* li) { return piece_fn(p, in, d_out, done, m, li); });
}

int trace_rays_locked(rb_engine* e, bool device, const rb_ray* rays, const uint32_t* seeds, size_t n, uint32_t first_sample, uint32_t samples,
                      rb_radiance* out) {
    return run_family(e, device, "radiance", RB_TRACE_PIECE_ITEMS, n, samples,
                      {FAMILY_ARRAY(rays, e->q_rays, 16, "d_rays"), FAMILY_ARRAY(seeds, e->rad_seeds, 4, "d_seeds")},
                      FAMILY_ARRAY(out, e->rad_out, 16, "d_out"), [&](size_t piece) { return radiance_scratch(e, piece, samples, false); },
                      [&](const rb::KParams& p, const void* const* in, void* o, size_t done, size_t m, rb::LaunchInfo* li) {
                          const rb::RadArgs a = trace_args(e, static_cast<const rb_ray*>(in[0]), static_cast<const uint32_t*>(in[1]),
                                                           static_cast<rb_radiance*>(o), done, m, first_sample, samples);
                          return rb::launch_radiance(p, a, e->stream, li);
                      });
}

// ---- camera rays made on the device (rb_abi.h)
// one piece, queued: the generator into the record scratch, the k_cam kernel of the scene's walk over it, the sum into `out`
int camera_piece(rb_engine* e, const rb::KParams& p, const rb_camera_ex& cam, uint64_t first_pixel, size_t done, size_t m,
                 uint32_t first_sample, uint32_t samples, rb_radiance* out, rb::LaunchInfo* li) {
    rb::CamGenArgs g{};
    g.cam = cam;
    g.recs = e->q_rays.ptr;
    g.first_pixel = static_cast<uint32_t>(first_pixel + done);
    g.n = static_cast<uint32_t>(m);
    g.first_sample = first_sample;
    g.samples = samples;
    if (const int st = e->t_generator.timed(e->stream, [&] { return rb::launch_camera_rays(g, e->stream); })) return st;
    return rb::launch_radiance(p, trace_args(e, e->q_rays.ptr, nullptr, out, done, m, first_sample, samples), e->stream, li, true);
}

int trace_camera_locked(rb_engine* e, bool device, const rb_camera_ex& cam, uint64_t first_pixel, size_t n, uint32_t first_sample,
                        uint32_t samples, rb_radiance* out) {
    return run_family(e, device, "camera", RB_CAMERA_PIECE_ITEMS, n, samples, {}, FAMILY_ARRAY(out, e->rad_out, 16, "d_out"),
                      [&](size_t piece) { return radiance_scratch(e, piece, samples, true); },
                      [&](const rb::KParams& p, const void* const*, void* o, size_t done, size_t m, rb::LaunchInfo* li) {
                          return camera_piece(e, p, cam, first_pixel, done, m, first_sample, samples, static_cast<rb_radiance*>(o), li);
                      });
}

// ---- hemisphere rays made on the device (rb_abi.h)
// what a call of the family is, beside its buffers
struct HemiCall {
    rb_hemi_params prm;
    uint32_t first_sample, samples;
    bool openness;
};

rb::HemiGenArgs hemi_gen_args(const HemiCall& c, const rb_surfel* surfels, const uint32_t* ids, rb_ray* recs, size_t done, size_t m) {
    rb::HemiGenArgs g{};
    g.surfels = surfels;
    g.ids = ids;
    g.recs = recs;
    g.offset = c.prm.offset;
    g.radius = c.prm.radius;
    g.n = static_cast<uint32_t>(m);
    g.id_base = static_cast<uint32_t>(done);
    g.first_sample = c.first_sample;
    g.samples = c.samples;
    return g;
}

// the scratch of one piece of `piece` surfels beside the caller's arrays: records and colours (radiance), or records, bounds
// and result bytes in linear order (openness)
int hemi_scratch(rb_engine* e, const HemiCall& c, size_t piece) {
    if (!c.openness) return radiance_scratch(e, piece, c.samples, true);
    const size_t items = piece * c.samples;
    HIP_TRY(e, e->q_rays.reserve(items));
    HIP_TRY(e, e->q_tmax.reserve(items));
    HIP_TRY(e, e->q_occl.reserve(items));
    return RB_OK;
}

// one piece, queued: surfels [done, done + m) of the call, at `surfels` / `ids` in device memory, into `out` (rb_radiance or
// rb_openness records).  Radiance: the generator in item order, the k_cam kernel of the scene's walk, the sum.  Openness: the
// generator in linear order with the bounds beside, the k_occl kernel, the count.
int hemi_piece(rb_engine* e, const rb::KParams& p, const HemiCall& c, const rb_surfel* surfels, const uint32_t* ids, size_t done,
               size_t m, void* out, rb::LaunchInfo* li) {
    rb::HemiGenArgs g = hemi_gen_args(c, surfels, ids, e->q_rays.ptr, done, m);
    if (c.openness) {
        g.tmax = e->q_tmax.ptr;
        g.linear = 1u;
    }
    if (const int st = e->t_generator.timed(e->stream, [&] { return rb::launch_hemisphere_rays(g, e->stream); })) return st;
    if (!c.openness)
        return rb::launch_radiance(p, trace_args(e, e->q_rays.ptr, nullptr, static_cast<rb_radiance*>(out), done, m, c.first_sample, c.samples),
                                   e->stream, li, true);
    rb::OcclArgs a{};
    a.q.rays = e->q_rays.ptr;
    a.q.n = static_cast<uint32_t>(m * c.samples);
    a.tmax = e->q_tmax.ptr;
    a.out = e->q_occl.ptr;
    a.mask = c.prm.mask;
    if (const int st = rb::launch_occluded(p, a, e->stream, li)) return st;
    return rb::launch_hemisphere_count(e->q_occl.ptr, static_cast<uint32_t>(m), c.samples, static_cast<rb_openness*>(out), e->stream);
}

int hemisphere_locked(rb_engine* e, bool device, const HemiCall& c, const rb_surfel* surfels, const uint32_t* seeds, size_t n, void* out) {
    return run_family(e, device, "hemisphere", RB_HEMI_PIECE_ITEMS, n, c.samples,
                      {FAMILY_ARRAY(surfels, e->hemi_surfels, 16, "d_surfels"), FAMILY_ARRAY(seeds, e->rad_seeds, 4, "d_seeds")},
                      c.openness ? FAMILY_ARRAY(out, e->hemi_open, 8, "d_out") : FAMILY_ARRAY(out, e->rad_out, 16, "d_out"),
                      [&](size_t piece) { return hemi_scratch(e, c, piece); },
                      [&](const rb::KParams& p, const void* const* in, void* o, size_t done, size_t m, rb::LaunchInfo* li) {
                          return hemi_piece(e, p, c, static_cast<const rb_surfel*>(in[0]), static_cast<const uint32_t*>(in[1]), done, m, o, li);
                      });
}

// ---- direct light at surface points (rb_abi.h)
rb::EmitArgs emit_args(const rb::KParams& p) {
    rb::EmitArgs s{};
    s.tris = p.tris;
    s.meshes = p.meshes;
    s.spheres = p.spheres;
    s.lights = p.lights;
    s.n_tris = p.u.bvh_triangle_count;
    s.n_meshes = p.n_meshes;
    s.n_spheres = p.u.spheres_count;
    s.n_lights = p.n_lights;
    s.color_hash = p.u.color_hash_enabled;
    return s;
}

// The emitter table of the current scene, made if the last update left none: flags, offsets and the total on the engine's
// stream, one wait for the total that sizes the table, the scatter.  *built: this call made it.
int ensure_emitters(rb_engine* e, const rb::KParams& p, bool* built) {
    *built = false;
    if (e->emit_valid) return RB_OK;
    const rb::EmitArgs s = emit_args(p);
    const uint64_t total = rb::emitter_candidates(s);
    if (total > 0x7FFFFFFFull - 63ull) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "the emitter table takes at most 2^31 - 64 candidate primitives");
    HIP_TRY(e, e->emit_count.reserve(1));
    if (total > 0u) {
        const size_t bytes = rb::emitter_work_bytes(static_cast<uint32_t>(total));
        if (bytes == 0) return rb::fail(e, RB_ERR_DEVICE, "the emitter table's scan could not be sized");
        HIP_TRY(e, e->emit_work.reserve(bytes));
    }
    int st = rb::launch_emitter_count(s, e->emit_work.ptr, e->emit_count.ptr, e->stream);
    if (st) return rb::fail(e, RB_ERR_DEVICE, "emitter count launch failed: %s", hipGetErrorString(static_cast<hipError_t>(st)));
    uint32_t n = 0;
    HIP_TRY(e, hipMemcpyAsync(&n, e->emit_count.ptr, sizeof(n), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    if (n > RB_MAX_EMITTERS) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "the scene has %u emitters; at most 2^24 are taken", n);
    HIP_TRY(e, e->emit_table.reserve(std::max<size_t>(n, 1)));
    st = rb::launch_emitter_scatter(s, e->emit_work.ptr, e->emit_table.ptr, n, e->stream);
    if (st) return rb::fail(e, RB_ERR_DEVICE, "emitter scatter launch failed: %s", hipGetErrorString(static_cast<hipError_t>(st)));
    e->emit_n = n;
    e->emit_valid = true;
    *built = true;
    return RB_OK;
}

// n inclusive pick weights by power of the n records at d_em into d_cdf, over the engine's scratch; queued, nothing waits
int queue_emitter_cdf(rb_engine* e, const rb_emitter* d_em, uint32_t n, uint32_t* d_cdf) {
    const size_t bytes = rb::emitter_cdf_work_bytes(n);
    if (bytes == 0) return rb::fail(e, RB_ERR_DEVICE, "the pick table's scan could not be sized");
    HIP_TRY(e, e->emit_cdf_work.reserve(bytes));
    const int st = rb::launch_emitter_cdf(d_em, n, e->emit_cdf_work.ptr, d_cdf, e->stream);
    if (st) return rb::fail(e, RB_ERR_DEVICE, "pick table launch failed: %s", hipGetErrorString(static_cast<hipError_t>(st)));
    return RB_OK;
}

// The pick weights by power of the scene's emitter table, which stands (ensure_emitters): made if the last update left none,
// kept as long as the table.  *built: this call made them.
int ensure_emitter_cdf(rb_engine* e, bool* built) {
    *built = false;
    if (e->emit_cdf_valid) return RB_OK;
    HIP_TRY(e, e->emit_cdf.reserve(std::max<size_t>(e->emit_n, 1)));
    if (const int rc = queue_emitter_cdf(e, e->emit_table.ptr, e->emit_n, e->emit_cdf.ptr)) return rc;
    e->emit_cdf_valid = true;
    *built = true;
    return RB_OK;
}

// rb_scene_emitter_cdf in both forms, as scene_emitters_locked: the emitter table first, outside the events; the build of the
// weights, if there is one, between them; then the copies
int scene_emitter_cdf_locked(rb_engine* e, bool device, uint32_t* out, size_t capacity, size_t* count, uint32_t* d_count) {
    if (device) {
        int rc = capacity ? device_range(e, out, capacity * sizeof(uint32_t), 4, "d_out") : RB_OK;
        if (!rc) rc = device_range(e, d_count, sizeof(uint32_t), 4, "d_count");
        if (rc) return rc;
    }
    rb::KParams p{};
    if (const int rc = query_prologue(e, &p)) return rc;
    bool built = false;
    if (const int rc = ensure_emitters(e, p, &built)) return rc;
    HIP_TRY(e, e->t_query.begin(e->stream));
    if (const int rc = ensure_emitter_cdf(e, &built)) return rc;
    HIP_TRY(e, e->t_query.end(e->stream));
    if (!built) e->t_query.reset();   // the time is the build's: 0 when the weights stood
    e->last_query_kernel_name = "k_emit_quant";
    const size_t m = std::min<size_t>(e->emit_n, capacity);
    if (device) {
        if (m) HIP_TRY(e, hipMemcpyAsync(out, e->emit_cdf.ptr, m * sizeof(uint32_t), hipMemcpyDeviceToDevice, e->stream));
        HIP_TRY(e, hipMemcpyAsync(d_count, e->emit_count.ptr, sizeof(uint32_t), hipMemcpyDeviceToDevice, e->stream));
        return RB_OK;
    }
    if (m) {
        if (const int rc = query_copy_out(e, out, e->emit_cdf.ptr, m * sizeof(uint32_t), page_locked(out))) return rc;
    }
    *count = e->emit_n;
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return RB_OK;
}

// rb_scene_emitters in both forms: the build, if there is one, between the query's two events; then the copies
int scene_emitters_locked(rb_engine* e, bool device, rb_emitter* out, size_t capacity, size_t* count, uint32_t* d_count) {
    if (device) {
        int rc = capacity ? device_range(e, out, capacity * sizeof(rb_emitter), 16, "d_out") : RB_OK;
        if (!rc) rc = device_range(e, d_count, sizeof(uint32_t), 4, "d_count");
        if (rc) return rc;
    }
    rb::KParams p{};
    if (const int rc = query_prologue(e, &p)) return rc;
    bool built = false;
    HIP_TRY(e, e->t_query.begin(e->stream));
    if (const int rc = ensure_emitters(e, p, &built)) return rc;
    HIP_TRY(e, e->t_query.end(e->stream));
    if (!built) e->t_query.reset();   // the time is the build's: 0 when the table stood
    e->last_query_kernel_name = "k_emit_scatter";
    const size_t m = std::min<size_t>(e->emit_n, capacity);
    if (device) {
        if (m) HIP_TRY(e, hipMemcpyAsync(out, e->emit_table.ptr, m * sizeof(rb_emitter), hipMemcpyDeviceToDevice, e->stream));
        HIP_TRY(e, hipMemcpyAsync(d_count, e->emit_count.ptr, sizeof(uint32_t), hipMemcpyDeviceToDevice, e->stream));
        return RB_OK;
    }
    if (m) {
        if (const int rc = query_copy_out(e, out, e->emit_table.ptr, m * sizeof(rb_emitter), page_locked(out))) return rc;
    }
    *count = e->emit_n;
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return RB_OK;
}

// what a call of rb_direct_light is, beside its buffers: the table is in device memory by now
struct DirectCall {
    rb_light_params prm;
    uint32_t first_sample, samples;
    const rb_emitter* emitters;
    uint32_t n_emit;
    const uint32_t* cdf = nullptr;   // the pick weights of rb_direct_light_cdf, n_emit of them; nullptr: the uniform pick
    const rb_probe_grid* grid = nullptr;   // rb_direct_light_grid: `cdf` holds one table of n_emit per cell of this grid (section 24)
    rb_grid_tally* tally = nullptr;        // rb_direct_light_grid_tally: rows * n_emit records in device memory, added to (section 25)
};

rb::LightGenArgs light_gen_args(const DirectCall& c, const rb_surfel* surfels, const uint32_t* ids, rb_ray* recs, float* tmax, float* contrib,
                                size_t done, size_t m) {
    rb::LightGenArgs g{};
    g.surfels = surfels;
    g.ids = ids;
    g.emitters = c.emitters;
    g.recs = recs;
    g.tmax = tmax;
    g.contrib = contrib;
    g.offset = c.prm.offset;
    g.shorten = c.prm.shorten;
    g.n_emit = c.n_emit;
    g.n = static_cast<uint32_t>(m);
    g.id_base = static_cast<uint32_t>(done);
    g.first_sample = c.first_sample;
    g.samples = c.samples;
    return g;
}

// A piece of fewer than 64 surfels is laid out in linear order: item order would pad it to a whole block, and one surfel at
// 4096 samples would generate, store and walk 64 times its items.
bool direct_linear(size_t m) { return m < 64; }
// the items of a piece of `piece` surfels: whole blocks of 64 in item order
size_t direct_items(size_t piece, uint32_t samples) { return (direct_linear(piece) ? piece : ((piece + 63) / 64) * 64) * samples; }

// the scratch of one piece beside the caller's arrays: records, bounds, result bytes and the radiance family's colours
int direct_scratch(rb_engine* e, size_t piece, uint32_t samples) {
    const size_t items = direct_items(piece, samples);
    HIP_TRY(e, e->q_rays.reserve(items));
    HIP_TRY(e, e->q_tmax.reserve(items));
    HIP_TRY(e, e->q_occl.reserve(items));
    HIP_TRY(e, e->rad_colors.reserve(items * 4));
    return RB_OK;
}

// one piece, queued: surfels [done, done + m) of the call, at `surfels` / `ids` in device memory, into out[m], as hemi_piece's
// openness branch has it but in item order (direct_linear: linear order): the generator, the k_occl kernel of the scene's walk
// over every record of the piece's blocks, the count of a tallied call (section 25), the fold (out == nullptr: a training-only
// call, none)
int direct_piece(rb_engine* e, const rb::KParams& p, const DirectCall& c, const rb_surfel* surfels, const uint32_t* ids, size_t done, size_t m,
                 rb_radiance* out, rb::LaunchInfo* li) {
    rb::LightGenArgs g = light_gen_args(c, surfels, ids, e->q_rays.ptr, e->q_tmax.ptr, e->rad_colors.ptr, done, m);
    g.linear = direct_linear(m) ? 1u : 0u;
    if (const int st = e->t_generator.timed(e->stream, [&] { return rb::launch_light_rays(g, e->stream, c.cdf, c.grid); })) return st;
    rb::OcclArgs a{};
    a.q.rays = e->q_rays.ptr;
    a.q.n = static_cast<uint32_t>(direct_items(m, c.samples));
    a.tmax = e->q_tmax.ptr;
    a.out = e->q_occl.ptr;
    a.mask = c.prm.mask;
    if (const int st = rb::launch_occluded(p, a, e->stream, li)) return st;
    if (c.tally && c.cdf && c.grid)
        if (const int st = rb::launch_grid_tally(g, c.cdf, *c.grid, e->q_occl.ptr, c.tally, e->stream)) return st;
    if (!out) return 0;
    return rb::launch_direct_fold(e->q_occl.ptr, e->rad_colors.ptr, static_cast<uint32_t>(m), c.samples, g.linear, out, e->stream);
}

// `weighted`: rb_direct_light_cdf -- the pick by `cdf`, the caller's n_emit weights, or (nullptr) by the table's power: the scene's
// kept weights for the scene's table, and for a caller's table weights made for this call in the engine's scratch, queued
int direct_light_locked(rb_engine* e, bool device, bool weighted, const rb_emitter* emitters, const uint32_t* cdf, size_t n_emit,
                        const rb_surfel* surfels, const uint32_t* seeds, size_t n, const rb_light_params& prm, uint32_t first_sample,
                        uint32_t samples, rb_radiance* out) {
    DirectCall c{prm, first_sample, samples, emitters, static_cast<uint32_t>(n_emit)};
    if (device) {   // every buffer of the caller's before anything is queued or the table is made: a refused call has done nothing
        int rc = device_range(e, surfels, n * sizeof(rb_surfel), 16, "d_surfels");
        if (!rc && seeds) rc = device_range(e, seeds, n * sizeof(uint32_t), 4, "d_seeds");
        if (!rc) rc = device_range(e, out, n * sizeof(rb_radiance), 16, "d_out");
        if (!rc && emitters && n_emit > 0) rc = device_range(e, emitters, n_emit * sizeof(rb_emitter), 16, "d_emitters");
        if (!rc && emitters && cdf && n_emit > 0) rc = device_range(e, cdf, n_emit * sizeof(uint32_t), 4, "d_cdf");
        if (rc) return rc;
    }
    if (!emitters) {   // the scene's own table
        rb::KParams p{};
        bool built = false;
        int rc = query_prologue(e, &p);
        if (!rc) rc = ensure_emitters(e, p, &built);
        if (rc) return rc;
        if (!rc && weighted) rc = ensure_emitter_cdf(e, &built);
        if (rc) return rc;
        c.emitters = e->emit_table.ptr;
        c.n_emit = e->emit_n;
        if (weighted) c.cdf = e->emit_cdf.ptr;
    } else if (!device) {   // a caller's table in host memory: staged once per call
        if (const int rc = require_ready(e)) return rc;
        HIP_TRY(e, e->emit_given.reserve(std::max<size_t>(n_emit, 1)));
        if (n_emit > 0) HIP_TRY(e, hipMemcpyAsync(e->emit_given.ptr, emitters, n_emit * sizeof(rb_emitter), hipMemcpyHostToDevice, e->stream));
        c.emitters = e->emit_given.ptr;
    } else if (weighted) {
        if (const int rc = require_ready(e)) return rc;
    }
    if (emitters && weighted && n_emit > 0) {   // a caller's table: its weights, or those its power gives, beside it
        if (device && cdf) {
            c.cdf = cdf;
        } else {
            HIP_TRY(e, e->emit_cdf_given.reserve(n_emit));
            if (cdf) HIP_TRY(e, hipMemcpyAsync(e->emit_cdf_given.ptr, cdf, n_emit * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
            else if (const int rc = queue_emitter_cdf(e, c.emitters, c.n_emit, e->emit_cdf_given.ptr)) return rc;
            c.cdf = e->emit_cdf_given.ptr;
        }
    }
    return run_family(e, device, "direct light", RB_HEMI_PIECE_ITEMS, n, samples,
                      {FAMILY_ARRAY(surfels, e->hemi_surfels, 16, "d_surfels"), FAMILY_ARRAY(seeds, e->rad_seeds, 4, "d_seeds")},
                      FAMILY_ARRAY(out, e->rad_out, 16, "d_out"), [&](size_t piece) { return direct_scratch(e, piece, samples); },
                      [&](const rb::KParams& p, const void* const* in, void* o, size_t done, size_t m, rb::LaunchInfo* li) {
                          return direct_piece(e, p, c, static_cast<const rb_surfel*>(in[0]), static_cast<const uint32_t*>(in[1]), done, m,
                                              static_cast<rb_radiance*>(o), li);
                      });
}

// ---- direct light with the emitters picked per grid cell (rb_abi.h)
size_t grid_cells(const rb_probe_grid& g) { return static_cast<size_t>(g.counts[0]) * g.counts[1] * g.counts[2]; }

// the tables of the n records at d_em over `grid` into d_tables, over the engine's scratch; queued, nothing waits
// (d_tally: the learned weight of section 25 with `prior`)
int queue_emitter_grid(rb_engine* e, const rb_emitter* d_em, uint32_t n, const rb_probe_grid& grid, uint32_t* d_tables,
                       const rb_grid_tally* d_tally = nullptr, float prior = 0.0f) {
    HIP_TRY(e, e->emit_grid_work.reserve(rb::emitter_grid_work_bytes(n)));
    const int st = rb::launch_emitter_grid(d_em, n, grid, e->emit_grid_work.ptr, d_tables, e->stream, d_tally, prior);
    if (st) return rb::fail(e, RB_ERR_DEVICE, "grid table launch failed: %s", hipGetErrorString(static_cast<hipError_t>(st)));
    return RB_OK;
}

// the scene's table for a call that names its length: the table, made if need be, and n_emit held to its count
int scene_emitters_counted(rb_engine* e, size_t n_emit) {
    rb::KParams p{};
    bool built = false;
    int rc = query_prologue(e, &p);
    if (!rc) rc = ensure_emitters(e, p, &built);
    if (rc) return rc;
    if (n_emit != e->emit_n) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "n_emit is %zu, the scene's table has %u emitters", n_emit, e->emit_n);
    return RB_OK;
}

// rb_emitter_grid_cdf_device: the caller's buffers, the scene's table where it is asked for -- outside the events --, the build;
// `learned`: rb_emitter_grid_learned_device, with the caller's tally and prior
int emitter_grid_device_locked(rb_engine* e, const rb_emitter* d_emitters, size_t n_emit, const rb_probe_grid& grid, uint32_t* d_tables,
                               bool learned = false, const rb_grid_tally* d_tally = nullptr, float prior = 0.0f) {
    int rc = n_emit > 0 ? device_range(e, d_tables, grid_cells(grid) * n_emit * sizeof(uint32_t), 4, "d_tables_out") : RB_OK;
    if (!rc && learned && n_emit > 0) rc = device_range(e, d_tally, grid_cells(grid) * n_emit * sizeof(rb_grid_tally), 4, "d_tally");
    if (!rc && d_emitters && n_emit > 0) rc = device_range(e, d_emitters, n_emit * sizeof(rb_emitter), 16, "d_emitters");
    if (!rc) rc = d_emitters ? query_prologue(e, nullptr) : scene_emitters_counted(e, n_emit);
    if (rc) return rc;
    e->last_query_kernel_name = learned ? "k_grid_rows_seen" : "k_grid_rows";
    if (n_emit == 0) return RB_OK;
    HIP_TRY(e, e->t_query.begin(e->stream));
    if ((rc = queue_emitter_grid(e, d_emitters ? d_emitters : e->emit_table.ptr, static_cast<uint32_t>(n_emit), grid, d_tables,
                                 learned ? d_tally : nullptr, prior)))
        return rc;
    HIP_TRY(e, e->t_query.end(e->stream));
    return RB_OK;
}

// rb_direct_light_grid in both forms: direct_light_locked with one table per cell, the caller's or made for this call; the
// pieces share them.  `tally`: rb_direct_light_grid_tally -- the caller's records, in device memory as they are, from host memory
// uploaded once, added to by every piece and downloaded at the end; `out` may then be nullptr
int direct_light_grid_locked(rb_engine* e, bool device, const rb_emitter* emitters, const rb_probe_grid& grid, const uint32_t* tables,
                             size_t n_emit, const rb_surfel* surfels, const uint32_t* seeds, size_t n, const rb_light_params& prm,
                             uint32_t first_sample, uint32_t samples, rb_radiance* out, rb_grid_tally* tally = nullptr) {
    DirectCall c{prm, first_sample, samples, emitters, static_cast<uint32_t>(n_emit)};
    c.grid = &grid;
    const size_t entries = grid_cells(grid) * n_emit;
    if (device) {   // every buffer of the caller's before anything is queued or a table is made: a refused call has done nothing
        int rc = device_range(e, surfels, n * sizeof(rb_surfel), 16, "d_surfels");
        if (!rc && seeds) rc = device_range(e, seeds, n * sizeof(uint32_t), 4, "d_seeds");
        if (!rc && (out || !tally)) rc = device_range(e, out, n * sizeof(rb_radiance), 16, "d_out");
        if (!rc && emitters && n_emit > 0) rc = device_range(e, emitters, n_emit * sizeof(rb_emitter), 16, "d_emitters");
        if (!rc && tables && entries > 0) rc = device_range(e, tables, entries * sizeof(uint32_t), 4, "d_tables");
        if (!rc && tally && entries > 0) rc = device_range(e, tally, entries * sizeof(rb_grid_tally), 4, "d_tally");
        if (rc) return rc;
    }
    if (!emitters) {   // the scene's own table
        if (const int rc = scene_emitters_counted(e, n_emit)) return rc;
        c.emitters = e->emit_table.ptr;
    } else {
        if (const int rc = require_ready(e)) return rc;
        if (!device) {   // a caller's table in host memory: staged once per call
            HIP_TRY(e, e->emit_given.reserve(std::max<size_t>(n_emit, 1)));
            if (n_emit > 0) HIP_TRY(e, hipMemcpyAsync(e->emit_given.ptr, emitters, n_emit * sizeof(rb_emitter), hipMemcpyHostToDevice, e->stream));
            c.emitters = e->emit_given.ptr;
        }
    }
    if (entries > 0) {
        if (device && tables) {
            c.cdf = tables;
        } else {
            HIP_TRY(e, e->emit_grid_tables.reserve(entries));
            if (tables) HIP_TRY(e, hipMemcpyAsync(e->emit_grid_tables.ptr, tables, entries * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
            else if (const int rc = queue_emitter_grid(e, c.emitters, c.n_emit, grid, e->emit_grid_tables.ptr)) return rc;
            c.cdf = e->emit_grid_tables.ptr;
        }
    }
    const bool staged_tally = tally && !device && entries > 0;
    if (tally && entries > 0) c.tally = tally;
    if (staged_tally) {
        HIP_TRY(e, e->emit_grid_tally.reserve(entries));
        HIP_TRY(e, hipMemcpyAsync(e->emit_grid_tally.ptr, tally, entries * sizeof(rb_grid_tally), hipMemcpyHostToDevice, e->stream));
        c.tally = e->emit_grid_tally.ptr;
    }
    const int rc = run_family(e, device, "direct light", RB_HEMI_PIECE_ITEMS, n, samples,
                              {FAMILY_ARRAY(surfels, e->hemi_surfels, 16, "d_surfels"), FAMILY_ARRAY(seeds, e->rad_seeds, 4, "d_seeds")},
                              FAMILY_ARRAY(out, e->rad_out, 16, "d_out"), [&](size_t piece) { return direct_scratch(e, piece, samples); },
                              [&](const rb::KParams& p, const void* const* in, void* o, size_t done, size_t m, rb::LaunchInfo* li) {
                                  return direct_piece(e, p, c, static_cast<const rb_surfel*>(in[0]), static_cast<const uint32_t*>(in[1]), done,
                                                      m, static_cast<rb_radiance*>(o), li);
                              });
    if (rc || !staged_tally) return rc;
    if (const int st = query_copy_out(e, tally, e->emit_grid_tally.ptr, entries * sizeof(rb_grid_tally), page_locked(tally))) return st;
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return RB_OK;
}

// ---- irradiance probes made on the device (rb_abi.h)
rb::ProbeGenArgs probe_gen_args(const rb_probe* probes, const uint32_t* ids, rb_ray* recs, size_t done, size_t m, uint32_t first_sample,
                                uint32_t samples) {
    rb::ProbeGenArgs g{};
    g.probes = probes;
    g.ids = ids;
    g.recs = recs;
    g.n = static_cast<uint32_t>(m);
    g.id_base = static_cast<uint32_t>(done);
    g.first_sample = first_sample;
    g.samples = samples;
    return g;
}

// the scratch of one piece of `piece` probes beside the caller's arrays: records, colours and the plain sums launch_radiance
// leaves beside them (not read)
int probe_scratch(rb_engine* e, size_t piece, uint32_t samples) {
    if (const int rc = radiance_scratch(e, piece, samples, true)) return rc;
    HIP_TRY(e, e->rad_out.reserve(piece));
    return RB_OK;
}

// one piece, queued: probes [done, done + m) of the call, at `probes` / `ids` in device memory, into out[m].  The generator in
// item order, the k_cam kernel of the scene's walk -- launch_radiance as every caller has it, its k_rad_sum included --, then
// the projection over the colour scratch and the records, which both stand until the next piece's generator.
int probe_piece(rb_engine* e, const rb::KParams& p, const rb_probe* probes, const uint32_t* ids, size_t done, size_t m,
                uint32_t first_sample, uint32_t samples, rb_sh9* out, rb::LaunchInfo* li) {
    const rb::ProbeGenArgs g = probe_gen_args(probes, ids, e->q_rays.ptr, done, m, first_sample, samples);
    if (const int st = e->t_generator.timed(e->stream, [&] { return rb::launch_probe_rays(g, e->stream); })) return st;
    if (const int st = rb::launch_radiance(p, trace_args(e, e->q_rays.ptr, nullptr, e->rad_out.ptr, done, m, first_sample, samples), e->stream, li, true))
        return st;
    return e->t_sh.timed(e->stream, [&] {
        return rb::launch_sh_project(e->rad_colors.ptr, e->q_rays.ptr, static_cast<uint32_t>(m), samples, out, 0u, e->stream);
    });
}

int probes_locked(rb_engine* e, bool device, const rb_probe* probes, const uint32_t* seeds, size_t n, uint32_t first_sample, uint32_t samples,
                  rb_sh9* out) {
    return run_family(e, device, "probe", RB_PROBE_PIECE_ITEMS, n, samples,
                      {FAMILY_ARRAY(probes, e->probe_pos, 16, "d_probes"), FAMILY_ARRAY(seeds, e->rad_seeds, 4, "d_seeds")},
                      FAMILY_ARRAY(out, e->probe_out, 16, "d_out"), [&](size_t piece) { return probe_scratch(e, piece, samples); },
                      [&](const rb::KParams& p, const void* const* in, void* o, size_t done, size_t m, rb::LaunchInfo* li) {
                          return probe_piece(e, p, static_cast<const rb_probe*>(in[0]), static_cast<const uint32_t*>(in[1]), done, m,
                                             first_sample, samples, static_cast<rb_sh9*>(o), li);
                      });
}

// ---- probe visibility: the depth bake (rb_abi.h)
// one piece, queued: probes [done, done + m) of the call into out[m], as hemi_piece's openness branch has it: the generator in
// linear order, the k_query kernel of the scene's walk over the records, the fold of the hits into the probes' maps
int depth_piece(rb_engine* e, const rb::KParams& p, const rb_probe* probes, const uint32_t* ids, size_t done, size_t m, uint32_t first_sample,
                uint32_t samples, float max_distance, rb_probe_depth* out, rb::LaunchInfo* li) {
    rb::ProbeGenArgs g = probe_gen_args(probes, ids, e->q_rays.ptr, done, m, first_sample, samples);
    g.linear = 1u;
    if (const int st = e->t_generator.timed(e->stream, [&] { return rb::launch_probe_rays(g, e->stream); })) return st;
    rb::QueryArgs q{};
    q.rays = e->q_rays.ptr;
    q.n = static_cast<uint32_t>(m * samples);
    q.hits = e->q_hits.ptr;
    if (const int st = rb::launch_query(p, q, e->stream, li)) return st;
    return e->t_depth.timed(e->stream, [&] {
        return rb::launch_depth_project(e->q_rays.ptr, e->q_hits.ptr, static_cast<uint32_t>(m), samples, max_distance, out, 0u, e->stream);
    });
}

// (probe, sample) items per piece: RB_DEPTH_PIECE_ITEMS in the environment (tests: a piece boundary at a few probes), else and
// at the most rb::kQueryPiece -- the records and the hits are rb_cast_rays' scratch
size_t depth_piece_items() {
    const char* const s = std::getenv("RB_DEPTH_PIECE_ITEMS");
    const unsigned long long v = s ? std::strtoull(s, nullptr, 10) : 0ull;
    return v ? static_cast<size_t>(std::min<unsigned long long>(v, rb::kQueryPiece)) : rb::kQueryPiece;
}

int probe_depth_locked(rb_engine* e, bool device, const rb_probe* probes, const uint32_t* seeds, size_t n, uint32_t first_sample, uint32_t samples,
                       float max_distance, rb_probe_depth* out) {
    return run_family(e, device, "probe depth", depth_piece_items(), n, samples,
                      {FAMILY_ARRAY(probes, e->probe_pos, 16, "d_probes"), FAMILY_ARRAY(seeds, e->rad_seeds, 4, "d_seeds")},
                      FAMILY_ARRAY(out, e->depth_out, 16, "d_out"),
                      [&](size_t piece) -> int {
                          HIP_TRY(e, e->q_rays.reserve(piece * samples));
                          HIP_TRY(e, e->q_hits.reserve(piece * samples));
                          return RB_OK;
                      },
                      [&](const rb::KParams& p, const void* const* in, void* o, size_t done, size_t m, rb::LaunchInfo* li) {
                          return depth_piece(e, p, static_cast<const rb_probe*>(in[0]), static_cast<const uint32_t*>(in[1]), done, m,
                                             first_sample, samples, max_distance, static_cast<rb_probe_depth*>(o), li);
                      });
}

// ---- refusals that several entry points share, each under the entry point's own name `who`; before a device is touched
int ray_count_check(rb_engine* e, const char* who, size_t n) {
    if (n > 0x7FFFFFFFull - 63ull) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s takes at most 2^31 - 64 rays per call", who);
    return RB_OK;
}

// `per`: what the samples are taken of, "ray" or "pixel"
int samples_check(rb_engine* e, const char* who, const char* per, uint32_t first_sample, uint32_t samples) {
    if (samples == 0 || samples > 65536u) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s takes 1 .. 65536 samples per %s, not %u", who, per, samples);
    if (static_cast<uint64_t>(first_sample) + samples > 0xFFFFFFFFull)
        return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: first_sample + samples = %u + %u does not fit 32 bits", who, first_sample, samples);
    return RB_OK;
}

// the refusals the two forms of rb_occluded share, the device form's under its own argument names
int occluded_check(rb_engine* e, const char* who, const char* null_text, const void* rays, size_t n, uint32_t mask, const void* out) {
    if (const int rc = ray_count_check(e, who, n)) return rc;
    if (mask > RB_MASK_ALL) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "mask has bits above RB_MASK_ALL");
    if (n > 0 && (!rays || !out)) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "%s", null_text);
    return RB_OK;
}

// the refusals the two forms of rb_trace_rays share
int trace_rays_check(rb_engine* e, const char* who, const void* rays, size_t n, uint32_t first_sample, uint32_t samples, const void* out) {
    int rc = samples_check(e, who, "ray", first_sample, samples);
    if (!rc) rc = ray_count_check(e, who, n);
    if (rc) return rc;
    if (n > 0 && (!rays || !out)) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: rays / out is NULL", who);
    return RB_OK;
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
    if (const int rc = samples_check(e, who, "pixel", first_sample, samples)) return rc;
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

// the refusals the two engine forms of rb_trace_camera share
int trace_camera_check(rb_engine* e, const char* who, const char* out_name, const rb_camera_ex* cam, uint64_t first_pixel, size_t n_pixels,
                       uint32_t first_sample, uint32_t samples, const void* out) {
    if (n_pixels > 0 && (!cam || !out)) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "%s: cam / %s is NULL", who, out_name);
    return cam ? camera_check(e, who, cam, first_pixel, n_pixels, first_sample, samples) : RB_OK;
}

// the refusals every hemisphere entry point shares; before a device is touched (e may be NULL: rb_hemisphere_rays)
int hemi_check(rb_engine* e, const char* who, const rb_hemi_params* prm, size_t n, uint32_t first_sample, uint32_t samples, bool openness) {
    if (const int rc = samples_check(e, who, "surfel", first_sample, samples)) return rc;
    if (n > 0x7FFFFFFFull - 63ull || static_cast<uint64_t>(n) * samples > 0x7FFFFFFFull - 63ull)
        return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s takes at most 2^31 - 64 surfels and (surfel, sample) items per call", who);
    if (!std::isfinite(prm->offset) || prm->offset < 0.0f) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: offset must be finite and at least 0", who);
    if (prm->flags != 0u) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: unknown flag bits 0x%x", who, prm->flags);
    for (const uint32_t r : prm->_reserved)
        if (r != 0u) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: _reserved must be 0", who);
    if (openness && std::isnan(prm->radius)) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: radius is NaN", who);
    if (openness && prm->mask > RB_MASK_ALL) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: mask has bits above RB_MASK_ALL", who);
    return RB_OK;
}

// the refusals every direct-light entry point shares; before a device is touched (e may be NULL: rb_light_rays, which reads no mask)
int light_check(rb_engine* e, const char* who, const rb_light_params* prm, size_t n_emit, size_t n, uint32_t first_sample, uint32_t samples,
                bool engine) {
    rb_hemi_params hp{};
    hp.offset = prm->offset;
    hp.flags = prm->flags;
    for (int k = 0; k < 4; k++) hp._reserved[k] = prm->_reserved[k];
    if (const int rc = hemi_check(e, who, &hp, n, first_sample, samples, false)) return rc;
    if (!std::isfinite(prm->shorten) || prm->shorten < 0.0f || prm->shorten > 0.5f)
        return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: shorten must be finite and 0 .. 0.5", who);
    if (engine && prm->mask > RB_MASK_ALL) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: mask has bits above RB_MASK_ALL", who);
    if (n_emit > RB_MAX_EMITTERS) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s takes at most 2^24 emitters", who);
    return RB_OK;
}

// a table of pick weights in host memory: inclusive sums, so non-decreasing, with a total of at most 2^24 (section 23.1)
int cdf_check(rb_engine* e, const char* who, const uint32_t* cdf, size_t n_emit) {
    if (n_emit > RB_MAX_EMITTERS) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s takes at most 2^24 emitters", who);
    for (size_t j = 1; j < n_emit; j++)
        if (cdf[j] < cdf[j - 1]) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: cdf[%zu] is below cdf[%zu]", who, j, j - 1);
    if (n_emit > 0 && cdf[n_emit - 1] > RB_MAX_EMITTERS) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: the cdf's total is above 2^24", who);
    return RB_OK;
}

// the refusals every probe entry point shares; before a device is touched (e may be NULL: rb_probe_rays)
int probe_check(rb_engine* e, const char* who, size_t n, uint32_t first_sample, uint32_t samples) {
    if (const int rc = samples_check(e, who, "probe", first_sample, samples)) return rc;
    if (n > 0x7FFFFFFFull - 63ull || static_cast<uint64_t>(n) * samples > 0x7FFFFFFFull - 63ull)
        return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s takes at most 2^31 - 64 probes and (probe, sample) items per call", who);
    return RB_OK;
}

// ---- light points from a baked probe grid (rb_abi.h)
// the refusals the forms of rb_probe_coefficients share; before a device is touched (e may be NULL: the engine-less form)
int probe_coeffs_check(rb_engine* e, const char* who, const void* sums, size_t n, const void* out) {
    if (n > 0x7FFFFFFFull - 63ull) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s takes at most 2^31 - 64 probes per call", who);
    if (n > 0 && (!sums || !out)) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "%s: sums / coeffs_out is NULL", who);
    return RB_OK;
}

// ... and those of rb_light_points
int light_points_check(rb_engine* e, const char* who, const rb_probe_grid* g, const void* coeffs, const void* points, size_t m, const void* out) {
    if (!g) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "%s: grid is NULL", who);
    if (g->flags != 0u || g->_pad0 != 0u || g->_pad1 != 0u) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: the grid's flags and pad words must be 0", who);
    uint64_t probes = 1;
    for (int a = 0; a < 3; a++) {
        if (g->counts[a] == 0u) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: the grid has a count of 0", who);
        probes *= g->counts[a];   // (each factor is below 2^32 and the product is checked before the next: no wrap-around)
        if (probes > 0x7FFFFFFFull - 63ull) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s takes a grid of at most 2^31 - 64 probes", who);
        if (!std::isfinite(g->origin[a])) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: the grid's origin is not finite", who);
        if (!std::isfinite(g->step[a]) || !(g->step[a] > 0.0f)) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: the grid's step must be finite and greater than 0", who);
    }
    if (m > 0x7FFFFFFFull - 63ull) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s takes at most 2^31 - 64 points per call", who);
    if (m > 0 && (!coeffs || !points || !out)) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "%s: coeffs / points / out is NULL", who);
    return RB_OK;
}

// the refusals the entry points of the pick per grid cell share (section 24), before a device is touched: a NULL grid,
// rb_light_points' of the grid, the entry cap
int emitter_grid_check(rb_engine* e, const char* who, const rb_probe_grid* g, size_t n_emit) {
    if (const int rc = light_points_check(e, who, g, nullptr, nullptr, 0, nullptr)) return rc;
    if (n_emit > RB_MAX_EMITTERS) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s takes at most 2^24 emitters", who);
    if (static_cast<uint64_t>(grid_cells(*g)) * std::max<size_t>(n_emit, 1) > RB_MAX_GRID_ENTRIES)
        return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: the grid's tables take at most 2^26 entries (cells times emitters)", who);
    return RB_OK;
}

// the prior of section 25: finite, 0 < a <= 2^24
int prior_check(rb_engine* e, const char* who, float prior) {
    if (!(std::isfinite(prior) && prior > 0.0f && prior <= 16777216.0f))
        return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: the prior must be finite, above 0 and at most 16777216", who);
    return RB_OK;
}

// tables in host memory: every row a table in cdf_check's sense
int grid_tables_check(rb_engine* e, const char* who, const rb_probe_grid& g, const uint32_t* tables, size_t n_emit) {
    for (size_t r = 0, rows = grid_cells(g); r < rows && n_emit > 0; r++)
        if (const int rc = cdf_check(e, who, tables + r * n_emit, n_emit)) return rc;
    return RB_OK;
}

size_t grid_probes(const rb_probe_grid& g) { return static_cast<size_t>(g.counts[0]) * g.counts[1] * g.counts[2]; }

// points per launch of the engine-less rb_light_points: RB_LIGHT_PIECE_POINTS in the environment (tests: a piece boundary at
// a few points), else 2^22 -- 128 + 64 MiB of scratch
size_t light_piece_points() {
    const char* const s = std::getenv("RB_LIGHT_PIECE_POINTS");
    const unsigned long long v = s ? std::strtoull(s, nullptr, 10) : 0ull;
    return v ? static_cast<size_t>(std::min<unsigned long long>(v, 0x7FFFFFFFull - 63ull)) : size_t(1) << 22;
}

int probe_coeffs_device_locked(rb_engine* e, const rb_sh9* d_sums, size_t n, rb_sh9* d_out) {
    int rc = device_range(e, d_sums, n * sizeof(rb_sh9), 16, "d_sums");
    if (!rc) rc = device_range(e, d_out, n * sizeof(rb_sh9), 16, "d_coeffs_out");
    if (rc) return rc;
    return device_stream_locked(e, [&](rb::LaunchInfo* li) {
        li->kernel_name = "k_probe_coeffs";
        return rb::launch_probe_coeffs(d_sums, static_cast<uint32_t>(n), d_out, e->stream);
    });
}

int light_points_device_locked(rb_engine* e, const rb_probe_grid& g, const rb_sh9* d_coeffs, const rb_surfel* d_points, size_t m, rb_lit* d_out) {
    int rc = device_range(e, d_coeffs, grid_probes(g) * sizeof(rb_sh9), 16, "d_coeffs");
    if (!rc) rc = device_range(e, d_points, m * sizeof(rb_surfel), 16, "d_points");
    if (!rc) rc = device_range(e, d_out, m * sizeof(rb_lit), 16, "d_out");
    if (rc) return rc;
    return device_stream_locked(e, [&](rb::LaunchInfo* li) {
        return rb::launch_probe_light(rb::ProbeLightArgs{g, d_coeffs, d_points, d_out, static_cast<uint32_t>(m)}, 0u, e->stream, &li->kernel_name);
    });
}

// ---- probe visibility: moments and the blend (rb_abi.h)
// the refusals the forms of rb_probe_moments share; before a device is touched (e may be NULL: the engine-less form)
int probe_moments_check(rb_engine* e, const char* who, const void* sums, size_t n, const void* out) {
    if (n > 0x7FFFFFFFull - 63ull) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s takes at most 2^31 - 64 probes per call", who);
    if (n > 0 && (!sums || !out)) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "%s: sums / moments_out is NULL", who);
    return RB_OK;
}

// ... and those of rb_light_points_visible: its own, then rb_light_points'
int light_visible_check(rb_engine* e, const char* who, const rb_probe_grid* g, const void* coeffs, const void* moments, const void* points,
                        size_t m, const rb_light_visibility* prm, const void* out) {
    if (!prm) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "%s: params is NULL", who);
    if (!std::isfinite(prm->normal_bias)) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: normal_bias is not finite", who);
    if (!(prm->min_visibility >= 0.0f && prm->min_visibility <= 1.0f)) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: min_visibility must be 0 .. 1", who);
    if ((prm->flags & ~static_cast<uint32_t>(RB_VIS_NO_WRAP | RB_VIS_NO_DEPTH)) != 0u) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: unknown flag bits 0x%x", who, prm->flags);
    if (prm->_pad != 0u) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: _pad must be 0", who);
    if (const int rc = light_points_check(e, who, g, coeffs, points, m, out)) return rc;
    if (m > 0 && !moments && (prm->flags & RB_VIS_NO_DEPTH) == 0u) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "%s: moments is NULL without RB_VIS_NO_DEPTH", who);
    return RB_OK;
}

int probe_moments_device_locked(rb_engine* e, const rb_probe_depth* d_sums, size_t n, rb_probe_depth* d_out, float* d_share) {
    int rc = device_range(e, d_sums, n * sizeof(rb_probe_depth), 16, "d_sums");
    if (!rc) rc = device_range(e, d_out, n * sizeof(rb_probe_depth), 16, "d_moments_out");
    if (!rc && d_share) rc = device_range(e, d_share, n * sizeof(float), 4, "d_backface_share_out");
    if (rc) return rc;
    return device_stream_locked(e, [&](rb::LaunchInfo* li) {
        li->kernel_name = "k_probe_moments";
        return rb::launch_probe_moments(d_sums, static_cast<uint32_t>(n), d_out, d_share, e->stream);
    });
}

int light_visible_device_locked(rb_engine* e, const rb_probe_grid& g, const rb_sh9* d_coeffs, const rb_probe_depth* d_moments,
                                const rb_surfel* d_points, size_t m, const rb_light_visibility& prm, rb_lit* d_out) {
    int rc = device_range(e, d_coeffs, grid_probes(g) * sizeof(rb_sh9), 16, "d_coeffs");
    if (!rc && d_moments) rc = device_range(e, d_moments, grid_probes(g) * sizeof(rb_probe_depth), 16, "d_moments");
    if (!rc) rc = device_range(e, d_points, m * sizeof(rb_surfel), 16, "d_points");
    if (!rc) rc = device_range(e, d_out, m * sizeof(rb_lit), 16, "d_out");
    if (rc) return rc;
    return device_stream_locked(e, [&](rb::LaunchInfo* li) {
        li->kernel_name = "k_probe_light_vis";
        return rb::launch_probe_light_vis(rb::ProbeLightArgs{g, d_coeffs, d_points, d_out, static_cast<uint32_t>(m)}, d_moments, prm, e->stream);
    });
}

// ---- temporal reprojection (rb_abi.h)
int reproject_device_locked(rb_engine* e, const rb_reproject_params& prm, uint32_t w, uint32_t h, const rb_view& view, const float* d_prev4,
                            const rb_guide* d_prev_guides, const rb_guide* d_cur_guides, const float* d_cur4, float* d_out4) {
    const size_t n = static_cast<size_t>(w) * h;
    int rc = device_range(e, d_prev4, n * 16, 16, "d_prev4");
    if (!rc) rc = device_range(e, d_prev_guides, n * sizeof(rb_guide), 16, "d_prev_guides");
    if (!rc) rc = device_range(e, d_cur_guides, n * sizeof(rb_guide), 16, "d_cur_guides");
    if (!rc && d_cur4) rc = device_range(e, d_cur4, n * 16, 16, "d_cur4");
    if (!rc) rc = device_range(e, d_out4, n * 16, 16, "d_out4");
    if (rc) return rc;
    HIP_TRY(e, e->rp_planes.reserve(n * 24));   // the planes of the two guide arrays: scratch in stream order
    float* const planes = e->rp_planes.ptr;
    return device_stream_locked(e, [&](rb::LaunchInfo* li) {
        li->kernel_name = "k_reproject";
        rb::ReprojectArgs a{};
        a.w = w;
        a.h = h;
        a.view = view;
        a.prev4 = d_prev4;
        a.prev = rb::GuidePlanes{planes, planes + n * 4, planes + n * 8};
        a.cur = rb::GuidePlanes{planes + n * 12, planes + n * 16, planes + n * 20};
        a.cur4 = d_cur4;
        a.out4 = d_out4;
        if (const int st = rb::launch_guide_split(d_prev_guides, n, a.prev, e->stream)) return st;
        if (const int st = rb::launch_guide_split(d_cur_guides, n, a.cur, e->stream)) return st;
        return rb::launch_reproject(prm, a, e->stream);
    });
}

// the engine that answers a query (a multi-device handle: devices[0], which holds the whole scene) ...
rb_engine* query_engine(rb_engine* e) { return rb::is_group(e) ? e->parts[0].get() : e; }

// ... made current
rb_engine* answering(rb_engine* e) {
    rb_engine* const t = query_engine(e);
    rb::set_device(t);
    return t;
}

// a getter of one of the query's stage times: the lock, the engine that answers, the read
int query_stage_ms(rb_engine* e, rb::StageTimer rb_engine::*timer, float* ms) {
    if (!e || !ms) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    rb_engine* const t = query_engine(e);
    return stage_ms(e, t, t->*timer, ms);
}

int answered(rb_engine* e, rb_engine* t, int rc) {
    if (rc && t != e) copy_error(e, t);
    return rc;
}

// The one shape of an engine entry point: a NULL handle, the lock, `check()` -- the refusals that need no device, recorded on
// the handle --, the answering engine t made current, `run(t)`, its error copied to the handle.
template <class Check, class Run>
int engine_entry(rb_engine* e, Check&& check, Run&& run) {
    if (!e) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    if (const int rc = check()) return rc;
    rb_engine* const t = answering(e);
    return answered(e, t, run(t));
}

// ... of n items: an empty call asks for a ready engine and does nothing else, in every form (section 11.1)
template <class Check, class Run>
int engine_entry(rb_engine* e, size_t n, Check&& check, Run&& run) {
    return engine_entry(e, check, [&](rb_engine* t) { return n == 0 ? require_ready(t) : run(t); });
}

// the four engine entry points of the hemisphere family
int hemisphere_entry(rb_engine* e, const char* who, bool openness, bool device, const rb_surfel* surfels, const uint32_t* seeds, size_t n,
                     const rb_hemi_params* prm, uint32_t first_sample, uint32_t samples, void* out) {
    return engine_entry(
        e, n,
        [&] {
            if (n > 0 && (!surfels || !prm || !out)) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "%s: surfels / params / out is NULL", who);
            return prm ? hemi_check(e, who, prm, n, first_sample, samples, openness) : RB_OK;
        },
        [&](rb_engine* t) { return hemisphere_locked(t, device, HemiCall{*prm, first_sample, samples, openness}, surfels, seeds, n, out); });
}

// the four engine entry points of rb_direct_light; emitters == nullptr: the scene's own table, and n_emit is not looked at.
// `weighted`: the _cdf forms, whose table of weights must come with a table of emitters; one in host memory is looked at here
int direct_light_entry(rb_engine* e, const char* who, bool device, bool weighted, const rb_emitter* emitters, const uint32_t* cdf, size_t n_emit,
                       const rb_surfel* surfels, const uint32_t* seeds, size_t n, const rb_light_params* prm, uint32_t first_sample,
                       uint32_t samples, rb_radiance* out) {
    return engine_entry(
        e, n,
        [&] {
            if (n > 0 && (!surfels || !prm || !out)) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "%s: surfels / params / out is NULL", who);
            if (prm)
                if (const int rc = light_check(e, who, prm, emitters ? n_emit : 0, n, first_sample, samples, true)) return rc;
            if (cdf && !emitters) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: a cdf without emitters (the scene's table has the scene's own)", who);
            return (cdf && !device) ? cdf_check(e, who, cdf, n_emit) : RB_OK;
        },
        [&](rb_engine* t) {
            return direct_light_locked(t, device, weighted, emitters, cdf, n_emit, surfels, seeds, n, *prm, first_sample, samples, out);
        });
}

// the two engine entry points of rb_direct_light_grid; tables in host memory are looked at here.  `tallied`: those of
// rb_direct_light_grid_tally, which need a tally and may leave out `out`
int direct_light_grid_entry(rb_engine* e, const char* who, bool device, const rb_emitter* emitters, const rb_probe_grid* grid,
                            const uint32_t* tables, size_t n_emit, const rb_surfel* surfels, const uint32_t* seeds, size_t n,
                            const rb_light_params* prm, uint32_t first_sample, uint32_t samples, rb_radiance* out, bool tallied = false,
                            rb_grid_tally* tally = nullptr) {
    return engine_entry(
        e, n,
        [&] {
            if (tallied && !tally) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "%s: tally is NULL", who);
            if (n > 0 && (!surfels || !prm || (!out && !tallied)))
                return rb::fail(e, RB_ERR_NULL_ARGUMENT, "%s: surfels / params / out is NULL", who);
            if (prm)
                if (const int rc = light_check(e, who, prm, n_emit, n, first_sample, samples, true)) return rc;
            if (const int rc = emitter_grid_check(e, who, grid, n_emit)) return rc;
            return (tables && !device) ? grid_tables_check(e, who, *grid, tables, n_emit) : RB_OK;
        },
        [&](rb_engine* t) {
            return direct_light_grid_locked(t, device, emitters, *grid, tables, n_emit, surfels, seeds, n, *prm, first_sample, samples, out,
                                            tally);
        });
}

// the two engine entry points of the probe family
int probes_entry(rb_engine* e, const char* who, bool device, const rb_probe* probes, const uint32_t* seeds, size_t n, uint32_t first_sample,
                 uint32_t samples, rb_sh9* out) {
    return engine_entry(
        e, n,
        [&] {
            if (n > 0 && (!probes || !out)) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "%s: probes / out is NULL", who);
            return probe_check(e, who, n, first_sample, samples);
        },
        [&](rb_engine* t) { return probes_locked(t, device, probes, seeds, n, first_sample, samples, out); });
}

// the two engine entry points of the depth bake
int probe_depth_entry(rb_engine* e, const char* who, bool device, const rb_probe* probes, const uint32_t* seeds, size_t n, uint32_t first_sample,
                      uint32_t samples, float max_distance, rb_probe_depth* out) {
    return engine_entry(
        e, n,
        [&] {
            if (n > 0 && (!probes || !out)) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "%s: probes / out is NULL", who);
            if (!std::isfinite(max_distance) || !(max_distance > 0.0f)) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: max_distance must be finite and greater than 0", who);
            return probe_check(e, who, n, first_sample, samples);
        },
        [&](rb_engine* t) { return probe_depth_locked(t, device, probes, seeds, n, first_sample, samples, max_distance, out); });
}

// ---- lightmap texels made on the device (rb_abi.h)
// the refusals every lightmap entry point shares; before a device is touched (e may be NULL: the engine-less forms)
int lightmap_size_check(rb_engine* e, const char* who, uint32_t width, uint32_t height, uint32_t dilate) {
    if (width == 0u || height == 0u || width > RB_LIGHTMAP_MAX_SIDE || height > RB_LIGHTMAP_MAX_SIDE)
        return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: an atlas of %u x %u texels; 1 .. %u each are taken", who, width, height, RB_LIGHTMAP_MAX_SIDE);
    if (static_cast<uint64_t>(width) * height > 0x7FFFFFFFull - 63ull)
        return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s takes at most 2^31 - 64 texels per call", who);
    if (dilate > RB_LIGHTMAP_MAX_DILATE) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: dilate is %u; at most %u passes are taken", who, dilate, RB_LIGHTMAP_MAX_DILATE);
    return RB_OK;
}

int lightmap_check(rb_engine* e, const char* who, const rb_lightmap_params* prm) {
    if (const int rc = lightmap_size_check(e, who, prm->width, prm->height, prm->dilate)) return rc;
    if (!std::isfinite(prm->offset) || prm->offset < 0.0f) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: offset must be finite and at least 0", who);
    if ((prm->flags & ~static_cast<uint32_t>(RB_LIGHTMAP_FLIP)) != 0u) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: unknown flag bits 0x%x", who, prm->flags);
    for (const uint32_t r : prm->_reserved)
        if (r != 0u) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: _reserved must be 0", who);
    return RB_OK;
}

// units per cover launch: RB_LIGHTMAP_PIECE_UNITS in the environment (tests: a piece boundary at a small atlas), else the default
uint64_t lightmap_piece_units() {
    const char* const s = std::getenv("RB_LIGHTMAP_PIECE_UNITS");
    return s ? std::strtoull(s, nullptr, 10) : 0ull;
}

rb::LmArgs lightmap_args(const rb_lightmap_params& prm, const rb::PrepTri* ptris, const rb::PrepTriShade* pshade, uint32_t n_tris,
                         const float* uvs, uint32_t n_uvs) {
    rb::LmArgs g{};
    g.ptris = ptris;
    g.pshade = pshade;
    g.uvs = uvs;
    g.n_tris = n_tris;
    g.n_uvs = n_uvs;
    g.width = prm.width;
    g.height = prm.height;
    g.mesh = prm.mesh;
    g.flags = prm.flags;
    return g;
}

// triangles -> records in triangle order by the upload's own kernel, then the atlas; returns a HIP status
int lightmap_generate(const rb_lightmap_params& prm, const rb_gpu_triangle* d_tris, uint32_t n_tris, uint32_t tri_count, const float* d_uvs,
                      uint32_t n_uvs, uint32_t* d_iota, rb::PrepTri* d_ptris, rb::PrepTriShade* d_pshade, void* d_work, rb_surfel* d_surfels,
                      uint32_t* d_owners, hipStream_t stream) {
    if (n_tris > 0u) {
        if (const int st = rb::launch_lightmap_iota(d_iota, n_tris, stream)) return st;
        if (const int st = rb::launch_prep_tris(d_tris, tri_count, d_iota, n_tris, d_ptris, d_pshade, stream)) return st;
    }
    return rb::lightmap_surfels(lightmap_args(prm, d_ptris, d_pshade, n_tris, d_uvs, n_uvs), d_surfels, d_owners, d_work, lightmap_piece_units(), stream);
}

// what a lightmap call begins with: the two stage times of the lightmap call before are gone (a query that is none leaves them)
void lightmap_times_reset(rb_engine* e) {
    e->t_lm_surfels.reset();
    e->t_lm_resolve.reset();
}

// the surfel stage over the engine's scene as a pair of its own timer, queued on the engine's stream
int lightmap_stage_surfels(rb_engine* e, const rb::KParams& p, const rb_lightmap_params& prm, rb_surfel* d_surfels, uint32_t* d_owners) {
    return e->t_lm_surfels.timed(e->stream, [&] {
        return lightmap_generate(prm, e->tris.ptr, e->sc.n_tris, p.u.bvh_triangle_count, e->uvs.ptr, e->sc.n_uvs, e->lm_iota.ptr, e->lm_ptris.ptr,
                                 e->lm_pshade.ptr, e->lm_work.ptr, d_surfels, d_owners, e->stream);
    });
}

// the scratch of the surfel stage beside the caller's buffers
int lightmap_scratch(rb_engine* e, size_t n, bool owners) {
    const uint32_t n_tris = e->sc.n_tris;
    HIP_TRY(e, e->lm_iota.reserve(n_tris));
    HIP_TRY(e, e->lm_ptris.reserve(n_tris));
    HIP_TRY(e, e->lm_pshade.reserve(n_tris));
    HIP_TRY(e, e->lm_work.reserve(rb::lightmap_work_bytes(n_tris)));
    if (owners) HIP_TRY(e, e->lm_owners.reserve(n));
    return RB_OK;
}

int lightmap_surfels_device_locked(rb_engine* e, const rb_lightmap_params& prm, rb_surfel* d_surfels, uint32_t* d_owners) {
    const size_t n = static_cast<size_t>(prm.width) * prm.height;
    int rc = device_range(e, d_surfels, n * sizeof(rb_surfel), 16, "d_surfels");
    if (!rc && d_owners) rc = device_range(e, d_owners, n * sizeof(uint32_t), 4, "d_owners");
    if (rc) return rc;
    lightmap_times_reset(e);
    return device_query_locked(e, [&](const rb::KParams& p, rb::LaunchInfo* li) {
        if (lightmap_scratch(e, n, d_owners == nullptr)) return static_cast<int>(hipErrorOutOfMemory);
        li->kernel_name = "k_lm_surfels";
        return lightmap_stage_surfels(e, p, prm, d_surfels, d_owners ? d_owners : e->lm_owners.ptr);
    });
}

// the three stages on the engine's stream into device buffers (either may be nullptr: the engine's scratch stands in); nothing
// is waited for but the surfel stage's unit total
int bake_lightmap_queue(rb_engine* e, const rb_lightmap_params& prm, uint32_t first_sample, uint32_t samples, float* d_rgba, rb_radiance* d_sums) {
    const size_t n = static_cast<size_t>(prm.width) * prm.height;
    rb_hemi_params hp{};
    hp.offset = prm.offset;
    const HemiCall c{hp, first_sample, samples, false};
    const size_t piece = piece_items(RB_HEMI_PIECE_ITEMS, n, samples);
    lightmap_times_reset(e);
    return device_query_locked(e, [&](const rb::KParams& p, rb::LaunchInfo* li) {
        hipError_t st = hipSuccess;
        if (lightmap_scratch(e, n, true) || hemi_scratch(e, c, piece)) return static_cast<int>(hipErrorOutOfMemory);
        st = e->lm_surfels.reserve(n);
        if (st == hipSuccess && !d_sums) st = e->lm_sums.reserve(n);
        if (st == hipSuccess && d_rgba && prm.dilate > 0u) st = e->lm_rgba[1].reserve(n * 4);
        if (st != hipSuccess) return static_cast<int>(st);
        rb_radiance* const sums = d_sums ? d_sums : e->lm_sums.ptr;
        if (const int s = lightmap_stage_surfels(e, p, prm, e->lm_surfels.ptr, e->lm_owners.ptr)) return s;
        if (const int s = for_pieces(n, piece, [&](size_t done, size_t m) {
                return hemi_piece(e, p, c, e->lm_surfels.ptr + done, nullptr, done, m, sums + done, li);
            }))
            return s;
        if (!d_rgba) return 0;
        return e->t_lm_resolve.timed(e->stream, [&] {
            return rb::launch_lightmap_resolve(sums, prm.width, prm.height, prm.dilate, d_rgba, e->lm_rgba[1].ptr, e->stream);
        });
    });
}

int bake_lightmap_device_locked(rb_engine* e, const rb_lightmap_params& prm, uint32_t first_sample, uint32_t samples, float* d_rgba, rb_radiance* d_sums) {
    const size_t n = static_cast<size_t>(prm.width) * prm.height;
    int rc = RB_OK;
    if (d_rgba) rc = device_range(e, d_rgba, n * 16, 16, "d_rgba_out");
    if (!rc && d_sums) rc = device_range(e, d_sums, n * sizeof(rb_radiance), 16, "d_sums_out");
    return rc ? rc : bake_lightmap_queue(e, prm, first_sample, samples, d_rgba, d_sums);
}

// the host form: the device form into the engine's own buffers, then the copies out and the wait
int bake_lightmap_locked(rb_engine* e, const rb_lightmap_params& prm, uint32_t first_sample, uint32_t samples, float* rgba_out, rb_radiance* sums_out) {
    const size_t n = static_cast<size_t>(prm.width) * prm.height;
    if (rgba_out) HIP_TRY(e, e->lm_rgba[0].reserve(n * 4));
    int rc = bake_lightmap_queue(e, prm, first_sample, samples, rgba_out ? e->lm_rgba[0].ptr : nullptr, nullptr);
    if (!rc && rgba_out) rc = query_copy_out(e, rgba_out, e->lm_rgba[0].ptr, n * 16, page_locked(rgba_out));
    if (!rc && sums_out) rc = query_copy_out(e, sums_out, e->lm_sums.ptr, n * sizeof(rb_radiance), page_locked(sums_out));
    if (rc) return rc;
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return RB_OK;
}

int bake_lightmap_entry(rb_engine* e, const char* who, bool device, const rb_lightmap_params* prm, uint32_t first_sample, uint32_t samples,
                        float* rgba, rb_radiance* sums) {
    return engine_entry(
        e,
        [&] {
            if (!prm || (!rgba && !sums)) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "%s: params is NULL, or rgba_out and sums_out both are", who);
            if (const int rc = lightmap_check(e, who, prm)) return rc;
            rb_hemi_params hp{};
            hp.offset = prm->offset;
            return hemi_check(e, who, &hp, static_cast<size_t>(prm->width) * prm->height, first_sample, samples, false);
        },
        [&](rb_engine* t) {
            return device ? bake_lightmap_device_locked(t, *prm, first_sample, samples, rgba, sums)
                          : bake_lightmap_locked(t, *prm, first_sample, samples, rgba, sums);
        });
}


// rb_light_rays, rb_light_rays_cdf (`weighted`: the pick by `cdf`, or by the table's power where it is NULL) and
// rb_light_rays_grid (`gridded`: `cdf` holds one table per cell of `grid`, or NULL: made here)
int light_rays_entry(const char* who, int32_t device, bool weighted, const rb_emitter* emitters, const uint32_t* cdf, size_t n_emit,
                     const rb_surfel* surfels, const uint32_t* seeds, size_t n, const rb_light_params* params, uint32_t first_sample,
                     uint32_t samples, rb_ray* rays_out, float* tmax_out, float* contrib_out, bool gridded = false,
                     const rb_probe_grid* grid = nullptr) {
    if ((n_emit > 0 && !emitters) || (n > 0 && (!surfels || !params || !rays_out || !tmax_out || !contrib_out)))
        return rb::fail(nullptr, RB_ERR_NULL_ARGUMENT, "%s: emitters / surfels / params / rays_out / tmax_out / contrib_out is NULL", who);
    if (params)
        if (const int rc = light_check(nullptr, who, params, n_emit, n, first_sample, samples, false)) return rc;
    if (gridded)
        if (const int rc = emitter_grid_check(nullptr, who, grid, n_emit)) return rc;
    if (cdf)
        if (const int rc = gridded ? grid_tables_check(nullptr, who, *grid, cdf, n_emit) : cdf_check(nullptr, who, cdf, n_emit)) return rc;
    if (n == 0) return RB_OK;
    const size_t piece = std::min(n, std::max<size_t>((size_t(1) << 22) / samples, 1));   // whole surfels, about 2^22 items
    const size_t entries = (gridded ? grid_cells(*grid) : 1) * n_emit;
    rb::DevBuf<rb_emitter> d_emit;
    rb::DevBuf<rb_surfel> d_surfels;
    rb::DevBuf<uint32_t> d_ids;
    rb::DevBuf<rb_ray> d_rays;
    rb::DevBuf<float> d_tmax, d_contrib;
    rb::DevBuf<uint32_t> d_cdf;
    rb::DevBuf<unsigned char> d_work;
    DeviceScope s(device);
    s.alloc(d_emit, std::max<size_t>(n_emit, 1));
    s.alloc(d_surfels, piece);
    if (seeds) s.alloc(d_ids, piece);
    s.alloc(d_rays, piece * samples);
    s.alloc(d_tmax, piece * samples);
    s.alloc(d_contrib, piece * samples * 4);
    s.upload(d_emit.ptr, emitters, n_emit * sizeof(rb_emitter));   // once per call
    if (weighted && n_emit > 0) {
        s.alloc(d_cdf, entries);
        if (cdf) {
            s.upload(d_cdf.ptr, cdf, entries * sizeof(uint32_t));
        } else if (gridded) {
            s.alloc(d_work, rb::emitter_grid_work_bytes(static_cast<uint32_t>(n_emit)));
            s.run([&] { return rb::launch_emitter_grid(d_emit.ptr, static_cast<uint32_t>(n_emit), *grid, d_work.ptr, d_cdf.ptr, s.stream); });
        } else {
            s.alloc(d_work, std::max<size_t>(rb::emitter_cdf_work_bytes(static_cast<uint32_t>(n_emit)), 256));
            s.run([&] { return rb::launch_emitter_cdf(d_emit.ptr, static_cast<uint32_t>(n_emit), d_work.ptr, d_cdf.ptr, s.stream); });
        }
    }
    const DirectCall c{*params, first_sample, samples, d_emit.ptr, static_cast<uint32_t>(n_emit), d_cdf.ptr, gridded ? grid : nullptr};
    for (size_t done = 0; done < n && s.ok(); done += piece) {
        const size_t m = std::min(piece, n - done), items = m * samples;
        s.upload(d_surfels.ptr, surfels + done, m * sizeof(rb_surfel));
        if (seeds) s.upload(d_ids.ptr, seeds + done, m * sizeof(uint32_t));
        rb::LightGenArgs g = light_gen_args(c, d_surfels.ptr, seeds ? d_ids.ptr : nullptr, d_rays.ptr, d_tmax.ptr, d_contrib.ptr, done, m);
        g.linear = 1u;
        s.run([&] { return rb::launch_light_rays(g, s.stream, c.cdf, c.grid); });
        s.download(rays_out + done * samples, d_rays.ptr, items * sizeof(rb_ray));
        s.download(tmax_out + done * samples, d_tmax.ptr, items * sizeof(float));
        s.download(contrib_out + done * samples * 4, d_contrib.ptr, items * 4 * sizeof(float));
        s.sync();   // the scratch is the next piece's
    }
    return s.finish(who);
}
// rb_emitter_grid_cdf, and (`learned`) rb_emitter_grid_learned with the caller's tally and prior
int emitter_grid_host(const char* who, int32_t device, const rb_emitter* emitters, size_t n_emit, const rb_probe_grid* grid, bool learned,
                      const rb_grid_tally* tally, float prior, uint32_t* tables_out) {
    if (!grid || (n_emit > 0 && (!emitters || !tables_out || (learned && !tally))))
        return rb::fail(nullptr, RB_ERR_NULL_ARGUMENT, "%s: grid / emitters / tally / tables_out is NULL", who);
    if (const int rc = emitter_grid_check(nullptr, who, grid, n_emit)) return rc;
    if (learned)
        if (const int rc = prior_check(nullptr, who, prior)) return rc;
    if (n_emit == 0) return RB_OK;
    const size_t entries = grid_cells(*grid) * n_emit;
    rb::DevBuf<rb_emitter> d_emit;
    rb::DevBuf<uint32_t> d_tables;
    rb::DevBuf<rb_grid_tally> d_tally;
    rb::DevBuf<unsigned char> d_work;
    DeviceScope s(device);
    s.alloc(d_emit, n_emit);
    s.alloc(d_tables, entries);
    if (learned) s.alloc(d_tally, entries);
    s.alloc(d_work, rb::emitter_grid_work_bytes(static_cast<uint32_t>(n_emit)));
    s.upload(d_emit.ptr, emitters, n_emit * sizeof(rb_emitter));
    if (learned) s.upload(d_tally.ptr, tally, entries * sizeof(rb_grid_tally));
    s.run([&] {
        return rb::launch_emitter_grid(d_emit.ptr, static_cast<uint32_t>(n_emit), *grid, d_work.ptr, d_tables.ptr, s.stream,
                                       learned ? d_tally.ptr : nullptr, prior);
    });
    s.download(tables_out, d_tables.ptr, entries * sizeof(uint32_t));
    return s.finish(who);
}

}  // namespace

extern "C" {

int rb_cast_rays(rb_engine* e, const rb_ray* rays, size_t n, rb_hit* hits_out, rb_surface* surf_out) {
    return engine_entry(
        e, n,
        [&]() -> int {
            if (const int rc = ray_count_check(e, "rb_cast_rays", n)) return rc;
            if (n > 0 && (!rays || !hits_out)) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "rays / hits_out is NULL");
            return RB_OK;
        },
        [&](rb_engine* t) { return cast_rays_locked(t, rays, n, hits_out, surf_out); });
}

int rb_render_hits(rb_engine* e, rb_hit* hits_out, rb_surface* surf_out) {
    return engine_entry(
        e, [&]() -> int { return hits_out ? RB_OK : rb::fail(e, RB_ERR_NULL_ARGUMENT, "hits_out is NULL"); },
        [&](rb_engine* t) {
            if (const int rc = require_ready(t)) return rc;
            // a multi-device handle: the whole frame on devices[0] (one ray per pixel is not worth a gather); a sharded engine: its own rows
            const bool sharded = t == e && t->opt.shard_count > 1;
            return pixel_hits_locked(t, 0, 0, t->sc.width, sharded ? t->sc.padded_rows : t->sc.height, !sharded, hits_out, surf_out);
        });
}

int rb_pick(rb_engine* e, uint32_t px, uint32_t py, rb_hit* hit_out, rb_surface* surf_out) {
    return engine_entry(
        e, [&]() -> int { return hit_out ? RB_OK : rb::fail(e, RB_ERR_NULL_ARGUMENT, "hit_out is NULL"); },
        [&](rb_engine* t) {
            if (const int rc = require_ready(t)) return rc;
            if (px >= t->sc.width || py >= t->sc.height)
                return rb::fail(t, RB_ERR_INVALID_OPTIONS, "pixel (%u, %u) is outside the %u x %u image", px, py, t->sc.width, t->sc.height);
            return pixel_hits_locked(t, px, py, 1, 1, true, hit_out, surf_out);
        });
}

int rb_occluded(rb_engine* e, const rb_ray* rays, const float* tmax, size_t n, uint32_t mask, uint8_t* out) {
    return engine_entry(
        e, n, [&] { return occluded_check(e, "rb_occluded", "rays / out is NULL", rays, n, mask, out); },
        [&](rb_engine* t) { return occluded_locked(t, rays, tmax, n, mask, out); });
}

int rb_occluded_device(rb_engine* e, const rb_ray* d_rays, const float* d_tmax, size_t n, uint32_t mask, uint8_t* d_out) {
    return engine_entry(
        e, n, [&] { return occluded_check(e, "rb_occluded_device", "d_rays / d_out is NULL", d_rays, n, mask, d_out); },
        [&](rb_engine* t) { return occluded_device_locked(t, d_rays, d_tmax, n, mask, d_out); });
}

int rb_cast_rays_device(rb_engine* e, const rb_ray* d_rays, size_t n, rb_hit* d_hits, rb_surface* d_surf) {
    return engine_entry(
        e, n,
        [&]() -> int {
            if (const int rc = ray_count_check(e, "rb_cast_rays_device", n)) return rc;
            if (n > 0 && (!d_rays || !d_hits)) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "d_rays / d_hits is NULL");
            return RB_OK;
        },
        [&](rb_engine* t) { return cast_rays_device_locked(t, d_rays, n, d_hits, d_surf); });
}

int rb_trace_rays(rb_engine* e, const rb_ray* rays, const uint32_t* seeds, size_t n, uint32_t first_sample, uint32_t samples,
                  rb_radiance* out) {
    return engine_entry(
        e, n, [&] { return trace_rays_check(e, "rb_trace_rays", rays, n, first_sample, samples, out); },
        [&](rb_engine* t) { return trace_rays_locked(t, false, rays, seeds, n, first_sample, samples, out); });
}

int rb_trace_rays_device(rb_engine* e, const rb_ray* d_rays, const uint32_t* d_seeds, size_t n, uint32_t first_sample,
                         uint32_t samples, rb_radiance* d_out) {
    return engine_entry(
        e, n, [&] { return trace_rays_check(e, "rb_trace_rays_device", d_rays, n, first_sample, samples, d_out); },
        [&](rb_engine* t) { return trace_rays_locked(t, true, d_rays, d_seeds, n, first_sample, samples, d_out); });
}

int rb_camera_rays(int32_t device, const rb_camera_ex* cam, uint64_t first_pixel, size_t n_pixels, uint32_t first_sample,
                   uint32_t samples, rb_ray* rays_out, uint32_t* seeds_out) {
    if (n_pixels > 0 && (!cam || !rays_out || !seeds_out)) return rb::fail(nullptr, RB_ERR_NULL_ARGUMENT, "cam / rays_out / seeds_out is NULL");
    if (cam)
        if (const int rc = camera_check(nullptr, "rb_camera_rays", cam, first_pixel, n_pixels, first_sample, samples)) return rc;
    if (n_pixels == 0) return RB_OK;
    const size_t items = n_pixels * samples, piece = std::min<size_t>(items, size_t(1) << 22);   // 128 + 16 MiB of scratch
    rb::DevBuf<rb_ray> d_rays;
    rb::DevBuf<uint32_t> d_seeds;
    DeviceScope s(device);
    s.alloc(d_rays, piece);
    s.alloc(d_seeds, piece);
    for (size_t done = 0; done < items && s.ok(); done += piece) {
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
        s.run([&] { return rb::launch_camera_rays(g, s.stream); });
        s.download(rays_out + done, d_rays.ptr, m * sizeof(rb_ray));
        s.download(seeds_out + done, d_seeds.ptr, m * sizeof(uint32_t));
        s.sync();   // the scratch is the next piece's
    }
    return s.finish("rb_camera_rays");
}

int rb_trace_camera(rb_engine* e, const rb_camera_ex* cam, uint64_t first_pixel, size_t n_pixels, uint32_t first_sample,
                    uint32_t samples, rb_radiance* out) {
    return engine_entry(
        e, n_pixels, [&] { return trace_camera_check(e, "rb_trace_camera", "out", cam, first_pixel, n_pixels, first_sample, samples, out); },
        [&](rb_engine* t) { return trace_camera_locked(t, false, *cam, first_pixel, n_pixels, first_sample, samples, out); });
}

int rb_trace_camera_device(rb_engine* e, const rb_camera_ex* cam, uint64_t first_pixel, size_t n_pixels, uint32_t first_sample,
                           uint32_t samples, rb_radiance* d_out) {
    return engine_entry(
        e, n_pixels,
        [&] { return trace_camera_check(e, "rb_trace_camera_device", "d_out", cam, first_pixel, n_pixels, first_sample, samples, d_out); },
        [&](rb_engine* t) { return trace_camera_locked(t, true, *cam, first_pixel, n_pixels, first_sample, samples, d_out); });
}

int rb_hemisphere_rays(int32_t device, const rb_surfel* surfels, const uint32_t* seeds, size_t n, const rb_hemi_params* params,
                       uint32_t first_sample, uint32_t samples, rb_ray* rays_out, uint32_t* seeds_out) {
    if (n > 0 && (!surfels || !params || !rays_out || !seeds_out))
        return rb::fail(nullptr, RB_ERR_NULL_ARGUMENT, "surfels / params / rays_out / seeds_out is NULL");
    if (params)
        if (const int rc = hemi_check(nullptr, "rb_hemisphere_rays", params, n, first_sample, samples, false)) return rc;
    if (n == 0) return RB_OK;
    const size_t piece = std::min(n, std::max<size_t>((size_t(1) << 22) / samples, 1));   // whole surfels, about 2^22 items
    rb::DevBuf<rb_surfel> d_surfels;
    rb::DevBuf<uint32_t> d_ids, d_seeds;
    rb::DevBuf<rb_ray> d_rays;
    DeviceScope s(device);
    s.alloc(d_surfels, piece);
    if (seeds) s.alloc(d_ids, piece);
    s.alloc(d_rays, piece * samples);
    s.alloc(d_seeds, piece * samples);
    const HemiCall c{*params, first_sample, samples, false};
    for (size_t done = 0; done < n && s.ok(); done += piece) {
        const size_t m = std::min(piece, n - done), items = m * samples;
        s.upload(d_surfels.ptr, surfels + done, m * sizeof(rb_surfel));
        if (seeds) s.upload(d_ids.ptr, seeds + done, m * sizeof(uint32_t));
        rb::HemiGenArgs g = hemi_gen_args(c, d_surfels.ptr, seeds ? d_ids.ptr : nullptr, d_rays.ptr, done, m);
        g.seeds = d_seeds.ptr;
        g.linear = 1u;
        s.run([&] { return rb::launch_hemisphere_rays(g, s.stream); });
        s.download(rays_out + done * samples, d_rays.ptr, items * sizeof(rb_ray));
        s.download(seeds_out + done * samples, d_seeds.ptr, items * sizeof(uint32_t));
        s.sync();   // the scratch is the next piece's
    }
    return s.finish("rb_hemisphere_rays");
}

int rb_trace_hemisphere(rb_engine* e, const rb_surfel* surfels, const uint32_t* seeds, size_t n, const rb_hemi_params* params,
                        uint32_t first_sample, uint32_t samples, rb_radiance* out) {
    return hemisphere_entry(e, "rb_trace_hemisphere", false, false, surfels, seeds, n, params, first_sample, samples, out);
}

int rb_trace_hemisphere_device(rb_engine* e, const rb_surfel* d_surfels, const uint32_t* d_seeds, size_t n,
                               const rb_hemi_params* params, uint32_t first_sample, uint32_t samples, rb_radiance* d_out) {
    return hemisphere_entry(e, "rb_trace_hemisphere_device", false, true, d_surfels, d_seeds, n, params, first_sample, samples, d_out);
}

int rb_openness_hemisphere(rb_engine* e, const rb_surfel* surfels, const uint32_t* seeds, size_t n, const rb_hemi_params* params,
                           uint32_t first_sample, uint32_t samples, rb_openness* out) {
    return hemisphere_entry(e, "rb_openness_hemisphere", true, false, surfels, seeds, n, params, first_sample, samples, out);
}

int rb_openness_hemisphere_device(rb_engine* e, const rb_surfel* d_surfels, const uint32_t* d_seeds, size_t n,
                                  const rb_hemi_params* params, uint32_t first_sample, uint32_t samples, rb_openness* d_out) {
    return hemisphere_entry(e, "rb_openness_hemisphere_device", true, true, d_surfels, d_seeds, n, params, first_sample, samples, d_out);
}

int rb_scene_emitters(rb_engine* e, rb_emitter* out, size_t capacity, size_t* count) {
    return engine_entry(
        e,
        [&]() -> int {
            if (!count || (capacity > 0 && !out)) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "rb_scene_emitters: count is NULL, or out with a capacity above 0");
            return RB_OK;
        },
        [&](rb_engine* t) { return scene_emitters_locked(t, false, out, capacity, count, nullptr); });
}

int rb_scene_emitters_device(rb_engine* e, rb_emitter* d_out, size_t capacity, uint32_t* d_count) {
    return engine_entry(
        e,
        [&]() -> int {
            if (!d_count || (capacity > 0 && !d_out))
                return rb::fail(e, RB_ERR_NULL_ARGUMENT, "rb_scene_emitters_device: d_count is NULL, or d_out with a capacity above 0");
            return RB_OK;
        },
        [&](rb_engine* t) { return scene_emitters_locked(t, true, d_out, capacity, nullptr, d_count); });
}

int rb_scene_emitter_cdf(rb_engine* e, uint32_t* out, size_t capacity, size_t* count) {
    return engine_entry(
        e,
        [&]() -> int {
            if (!count || (capacity > 0 && !out)) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "rb_scene_emitter_cdf: count is NULL, or out with a capacity above 0");
            return RB_OK;
        },
        [&](rb_engine* t) { return scene_emitter_cdf_locked(t, false, out, capacity, count, nullptr); });
}

int rb_scene_emitter_cdf_device(rb_engine* e, uint32_t* d_out, size_t capacity, uint32_t* d_count) {
    return engine_entry(
        e,
        [&]() -> int {
            if (!d_count || (capacity > 0 && !d_out))
                return rb::fail(e, RB_ERR_NULL_ARGUMENT, "rb_scene_emitter_cdf_device: d_count is NULL, or d_out with a capacity above 0");
            return RB_OK;
        },
        [&](rb_engine* t) { return scene_emitter_cdf_locked(t, true, d_out, capacity, nullptr, d_count); });
}

int rb_emitter_cdf(int32_t device, const rb_emitter* emitters, size_t n_emit, uint32_t* cdf_out) {
    if (n_emit > 0 && (!emitters || !cdf_out)) return rb::fail(nullptr, RB_ERR_NULL_ARGUMENT, "rb_emitter_cdf: emitters / cdf_out is NULL");
    if (n_emit > RB_MAX_EMITTERS) return rb::fail(nullptr, RB_ERR_INVALID_OPTIONS, "rb_emitter_cdf takes at most 2^24 emitters");
    if (n_emit == 0) return RB_OK;
    rb::DevBuf<rb_emitter> d_emit;
    rb::DevBuf<uint32_t> d_cdf;
    rb::DevBuf<unsigned char> d_work;
    DeviceScope s(device);
    s.alloc(d_emit, n_emit);
    s.alloc(d_cdf, n_emit);
    s.alloc(d_work, std::max<size_t>(rb::emitter_cdf_work_bytes(static_cast<uint32_t>(n_emit)), 256));
    s.upload(d_emit.ptr, emitters, n_emit * sizeof(rb_emitter));
    s.run([&] { return rb::launch_emitter_cdf(d_emit.ptr, static_cast<uint32_t>(n_emit), d_work.ptr, d_cdf.ptr, s.stream); });
    s.download(cdf_out, d_cdf.ptr, n_emit * sizeof(uint32_t));
    return s.finish("rb_emitter_cdf");
}


int rb_light_rays(int32_t device, const rb_emitter* emitters, size_t n_emit, const rb_surfel* surfels, const uint32_t* seeds, size_t n,
                  const rb_light_params* params, uint32_t first_sample, uint32_t samples, rb_ray* rays_out, float* tmax_out, float* contrib_out) {
    return light_rays_entry("rb_light_rays", device, false, emitters, nullptr, n_emit, surfels, seeds, n, params, first_sample, samples, rays_out,
                            tmax_out, contrib_out);
}

int rb_light_rays_cdf(int32_t device, const rb_emitter* emitters, const uint32_t* cdf, size_t n_emit, const rb_surfel* surfels,
                      const uint32_t* seeds, size_t n, const rb_light_params* params, uint32_t first_sample, uint32_t samples, rb_ray* rays_out,
                      float* tmax_out, float* contrib_out) {
    return light_rays_entry("rb_light_rays_cdf", device, true, emitters, cdf, n_emit, surfels, seeds, n, params, first_sample, samples, rays_out,
                            tmax_out, contrib_out);
}

int rb_direct_light(rb_engine* e, const rb_emitter* emitters, size_t n_emit, const rb_surfel* surfels, const uint32_t* seeds, size_t n,
                    const rb_light_params* params, uint32_t first_sample, uint32_t samples, rb_radiance* out) {
    return direct_light_entry(e, "rb_direct_light", false, false, emitters, nullptr, n_emit, surfels, seeds, n, params, first_sample, samples, out);
}

int rb_direct_light_device(rb_engine* e, const rb_emitter* d_emitters, size_t n_emit, const rb_surfel* d_surfels, const uint32_t* d_seeds,
                           size_t n, const rb_light_params* params, uint32_t first_sample, uint32_t samples, rb_radiance* d_out) {
    return direct_light_entry(e, "rb_direct_light_device", true, false, d_emitters, nullptr, n_emit, d_surfels, d_seeds, n, params, first_sample,
                              samples, d_out);
}

int rb_direct_light_cdf(rb_engine* e, const rb_emitter* emitters, const uint32_t* cdf, size_t n_emit, const rb_surfel* surfels,
                        const uint32_t* seeds, size_t n, const rb_light_params* params, uint32_t first_sample, uint32_t samples, rb_radiance* out) {
    return direct_light_entry(e, "rb_direct_light_cdf", false, true, emitters, cdf, n_emit, surfels, seeds, n, params, first_sample, samples, out);
}

int rb_direct_light_cdf_device(rb_engine* e, const rb_emitter* d_emitters, const uint32_t* d_cdf, size_t n_emit, const rb_surfel* d_surfels,
                               const uint32_t* d_seeds, size_t n, const rb_light_params* params, uint32_t first_sample, uint32_t samples,
                               rb_radiance* d_out) {
    return direct_light_entry(e, "rb_direct_light_cdf_device", true, true, d_emitters, d_cdf, n_emit, d_surfels, d_seeds, n, params, first_sample,
                              samples, d_out);
}

int rb_emitter_grid_cdf(int32_t device, const rb_emitter* emitters, size_t n_emit, const rb_probe_grid* grid, uint32_t* tables_out) {
    return emitter_grid_host("rb_emitter_grid_cdf", device, emitters, n_emit, grid, false, nullptr, 0.0f, tables_out);
}

int rb_emitter_grid_learned(int32_t device, const rb_emitter* emitters, size_t n_emit, const rb_probe_grid* grid, const rb_grid_tally* tally,
                            float prior, uint32_t* tables_out) {
    return emitter_grid_host("rb_emitter_grid_learned", device, emitters, n_emit, grid, true, tally, prior, tables_out);
}

int rb_emitter_grid_learned_device(rb_engine* e, const rb_emitter* d_emitters, size_t n_emit, const rb_probe_grid* grid,
                                   const rb_grid_tally* d_tally, float prior, uint32_t* d_tables_out) {
    return engine_entry(
        e,
        [&]() -> int {
            if (!grid || (n_emit > 0 && (!d_tables_out || !d_tally)))
                return rb::fail(e, RB_ERR_NULL_ARGUMENT, "rb_emitter_grid_learned_device: grid / d_tally / d_tables_out is NULL");
            if (const int rc = emitter_grid_check(e, "rb_emitter_grid_learned_device", grid, n_emit)) return rc;
            return prior_check(e, "rb_emitter_grid_learned_device", prior);
        },
        [&](rb_engine* t) { return emitter_grid_device_locked(t, d_emitters, n_emit, *grid, d_tables_out, true, d_tally, prior); });
}

int rb_emitter_grid_cdf_device(rb_engine* e, const rb_emitter* d_emitters, size_t n_emit, const rb_probe_grid* grid, uint32_t* d_tables_out) {
    return engine_entry(
        e,
        [&]() -> int {
            if (!grid || (n_emit > 0 && !d_tables_out)) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "rb_emitter_grid_cdf_device: grid / d_tables_out is NULL");
            return emitter_grid_check(e, "rb_emitter_grid_cdf_device", grid, n_emit);
        },
        [&](rb_engine* t) { return emitter_grid_device_locked(t, d_emitters, n_emit, *grid, d_tables_out); });
}

int rb_light_rays_grid(int32_t device, const rb_emitter* emitters, const rb_probe_grid* grid, const uint32_t* tables, size_t n_emit,
                       const rb_surfel* surfels, const uint32_t* seeds, size_t n, const rb_light_params* params, uint32_t first_sample,
                       uint32_t samples, rb_ray* rays_out, float* tmax_out, float* contrib_out) {
    return light_rays_entry("rb_light_rays_grid", device, true, emitters, tables, n_emit, surfels, seeds, n, params, first_sample, samples, rays_out,
                            tmax_out, contrib_out, true, grid);
}

int rb_direct_light_grid(rb_engine* e, const rb_emitter* emitters, const rb_probe_grid* grid, const uint32_t* tables, size_t n_emit,
                         const rb_surfel* surfels, const uint32_t* seeds, size_t n, const rb_light_params* params, uint32_t first_sample,
                         uint32_t samples, rb_radiance* out) {
    return direct_light_grid_entry(e, "rb_direct_light_grid", false, emitters, grid, tables, n_emit, surfels, seeds, n, params, first_sample, samples,
                                   out);
}

int rb_direct_light_grid_device(rb_engine* e, const rb_emitter* d_emitters, const rb_probe_grid* grid, const uint32_t* d_tables, size_t n_emit,
                                const rb_surfel* d_surfels, const uint32_t* d_seeds, size_t n, const rb_light_params* params,
                                uint32_t first_sample, uint32_t samples, rb_radiance* d_out) {
    return direct_light_grid_entry(e, "rb_direct_light_grid_device", true, d_emitters, grid, d_tables, n_emit, d_surfels, d_seeds, n, params,
                                   first_sample, samples, d_out);
}

int rb_direct_light_grid_tally(rb_engine* e, const rb_emitter* emitters, const rb_probe_grid* grid, const uint32_t* tables, size_t n_emit,
                               const rb_surfel* surfels, const uint32_t* seeds, size_t n, const rb_light_params* params,
                               uint32_t first_sample, uint32_t samples, rb_radiance* out, rb_grid_tally* tally) {
    return direct_light_grid_entry(e, "rb_direct_light_grid_tally", false, emitters, grid, tables, n_emit, surfels, seeds, n, params,
                                   first_sample, samples, out, true, tally);
}

int rb_direct_light_grid_tally_device(rb_engine* e, const rb_emitter* d_emitters, const rb_probe_grid* grid, const uint32_t* d_tables,
                                      size_t n_emit, const rb_surfel* d_surfels, const uint32_t* d_seeds, size_t n,
                                      const rb_light_params* params, uint32_t first_sample, uint32_t samples, rb_radiance* d_out,
                                      rb_grid_tally* d_tally) {
    return direct_light_grid_entry(e, "rb_direct_light_grid_tally_device", true, d_emitters, grid, d_tables, n_emit, d_surfels, d_seeds, n,
                                   params, first_sample, samples, d_out, true, d_tally);
}

int rb_probe_rays(int32_t device, const rb_probe* probes, const uint32_t* seeds, size_t n, uint32_t first_sample, uint32_t samples,
                  rb_ray* rays_out, uint32_t* seeds_out) {
    if (n > 0 && (!probes || !rays_out)) return rb::fail(nullptr, RB_ERR_NULL_ARGUMENT, "probes / rays_out is NULL");
    if (const int rc = probe_check(nullptr, "rb_probe_rays", n, first_sample, samples)) return rc;
    if (n == 0) return RB_OK;
    const size_t piece = std::min(n, std::max<size_t>((size_t(1) << 22) / samples, 1));   // whole probes, about 2^22 items
    rb::DevBuf<rb_probe> d_probes;
    rb::DevBuf<uint32_t> d_ids, d_seeds;
    rb::DevBuf<rb_ray> d_rays;
    DeviceScope s(device);
    s.alloc(d_probes, piece);
    if (seeds) s.alloc(d_ids, piece);
    s.alloc(d_rays, piece * samples);
    if (seeds_out) s.alloc(d_seeds, piece * samples);
    for (size_t done = 0; done < n && s.ok(); done += piece) {
        const size_t m = std::min(piece, n - done), items = m * samples;
        s.upload(d_probes.ptr, probes + done, m * sizeof(rb_probe));
        if (seeds) s.upload(d_ids.ptr, seeds + done, m * sizeof(uint32_t));
        rb::ProbeGenArgs g = probe_gen_args(d_probes.ptr, seeds ? d_ids.ptr : nullptr, d_rays.ptr, done, m, first_sample, samples);
        g.seeds = seeds_out ? d_seeds.ptr : nullptr;
        g.linear = 1u;
        s.run([&] { return rb::launch_probe_rays(g, s.stream); });
        s.download(rays_out + done * samples, d_rays.ptr, items * sizeof(rb_ray));
        if (seeds_out) s.download(seeds_out + done * samples, d_seeds.ptr, items * sizeof(uint32_t));
        s.sync();   // the scratch is the next piece's
    }
    return s.finish("rb_probe_rays");
}

int rb_bake_probes(rb_engine* e, const rb_probe* probes, const uint32_t* seeds, size_t n, uint32_t first_sample, uint32_t samples, rb_sh9* out) {
    return probes_entry(e, "rb_bake_probes", false, probes, seeds, n, first_sample, samples, out);
}

int rb_bake_probes_device(rb_engine* e, const rb_probe* d_probes, const uint32_t* d_seeds, size_t n, uint32_t first_sample,
                          uint32_t samples, rb_sh9* d_out) {
    return probes_entry(e, "rb_bake_probes_device", true, d_probes, d_seeds, n, first_sample, samples, d_out);
}

int rb_probe_coefficients(int32_t device, const rb_sh9* sums, size_t n, rb_sh9* coeffs_out) {
    if (const int rc = probe_coeffs_check(nullptr, "rb_probe_coefficients", sums, n, coeffs_out)) return rc;
    if (n == 0) return RB_OK;
    const size_t piece = std::min(n, size_t(1) << 22);   // 448 MiB of scratch at the most
    rb::DevBuf<rb_sh9> d_recs;
    DeviceScope s(device);
    s.alloc(d_recs, piece);
    for (size_t done = 0; done < n && s.ok(); done += piece) {
        const size_t m = std::min(piece, n - done);
        s.upload(d_recs.ptr, sums + done, m * sizeof(rb_sh9));
        s.run([&] { return rb::launch_probe_coeffs(d_recs.ptr, static_cast<uint32_t>(m), d_recs.ptr, s.stream); });
        s.download(coeffs_out + done, d_recs.ptr, m * sizeof(rb_sh9));
        s.sync();   // the scratch is the next piece's
    }
    return s.finish("rb_probe_coefficients");
}

int rb_probe_coefficients_device(rb_engine* e, const rb_sh9* d_sums, size_t n, rb_sh9* d_coeffs_out) {
    return engine_entry(
        e, n, [&] { return probe_coeffs_check(e, "rb_probe_coefficients_device", d_sums, n, d_coeffs_out); },
        [&](rb_engine* t) { return probe_coeffs_device_locked(t, d_sums, n, d_coeffs_out); });
}

int rb_light_points(int32_t device, const rb_probe_grid* grid, const rb_sh9* coeffs, const rb_surfel* points, size_t m, rb_lit* out) {
    if (const int rc = light_points_check(nullptr, "rb_light_points", grid, coeffs, points, m, out)) return rc;
    if (m == 0) return RB_OK;
    const size_t probes = grid_probes(*grid), piece = std::min(m, light_piece_points());
    rb::DevBuf<rb_sh9> d_coeffs;
    rb::DevBuf<rb_surfel> d_points;
    rb::DevBuf<rb_lit> d_out;
    DeviceScope s(device);
    s.alloc(d_coeffs, probes);
    s.alloc(d_points, piece);
    s.alloc(d_out, piece);
    s.upload(d_coeffs.ptr, coeffs, probes * sizeof(rb_sh9));   // once per call
    for (size_t done = 0; done < m && s.ok(); done += piece) {
        const size_t k = std::min(piece, m - done);
        s.upload(d_points.ptr, points + done, k * sizeof(rb_surfel));
        s.run([&] { return rb::launch_probe_light(rb::ProbeLightArgs{*grid, d_coeffs.ptr, d_points.ptr, d_out.ptr, static_cast<uint32_t>(k)}, 0u, s.stream); });
        s.download(out + done, d_out.ptr, k * sizeof(rb_lit));
        s.sync();   // the scratch is the next piece's
    }
    return s.finish("rb_light_points");
}

int rb_light_points_device(rb_engine* e, const rb_probe_grid* grid, const rb_sh9* d_coeffs, const rb_surfel* d_points, size_t m,
                           rb_lit* d_out) {
    return engine_entry(
        e, m, [&] { return light_points_check(e, "rb_light_points_device", grid, d_coeffs, d_points, m, d_out); },
        [&](rb_engine* t) { return light_points_device_locked(t, *grid, d_coeffs, d_points, m, d_out); });
}

int rb_bake_probe_depth(rb_engine* e, const rb_probe* probes, const uint32_t* seeds, size_t n, uint32_t first_sample, uint32_t samples,
                        float max_distance, rb_probe_depth* out) {
    return probe_depth_entry(e, "rb_bake_probe_depth", false, probes, seeds, n, first_sample, samples, max_distance, out);
}

int rb_bake_probe_depth_device(rb_engine* e, const rb_probe* d_probes, const uint32_t* d_seeds, size_t n, uint32_t first_sample,
                               uint32_t samples, float max_distance, rb_probe_depth* d_out) {
    return probe_depth_entry(e, "rb_bake_probe_depth_device", true, d_probes, d_seeds, n, first_sample, samples, max_distance, d_out);
}

int rb_probe_moments(int32_t device, const rb_probe_depth* sums, size_t n, rb_probe_depth* moments_out, float* backface_share_out) {
    if (const int rc = probe_moments_check(nullptr, "rb_probe_moments", sums, n, moments_out)) return rc;
    if (n == 0) return RB_OK;
    const size_t piece = std::min(n, size_t(1) << 18);   // 256 + 1 MiB of scratch at the most
    rb::DevBuf<rb_probe_depth> d_maps;
    rb::DevBuf<float> d_share;
    DeviceScope s(device);
    s.alloc(d_maps, piece);
    if (backface_share_out) s.alloc(d_share, piece);
    for (size_t done = 0; done < n && s.ok(); done += piece) {
        const size_t m = std::min(piece, n - done);
        s.upload(d_maps.ptr, sums + done, m * sizeof(rb_probe_depth));
        s.run([&] { return rb::launch_probe_moments(d_maps.ptr, static_cast<uint32_t>(m), d_maps.ptr, backface_share_out ? d_share.ptr : nullptr, s.stream); });
        s.download(moments_out + done, d_maps.ptr, m * sizeof(rb_probe_depth));
        if (backface_share_out) s.download(backface_share_out + done, d_share.ptr, m * sizeof(float));
        s.sync();   // the scratch is the next piece's
    }
    return s.finish("rb_probe_moments");
}

int rb_probe_moments_device(rb_engine* e, const rb_probe_depth* d_sums, size_t n, rb_probe_depth* d_moments_out, float* d_backface_share_out) {
    return engine_entry(
        e, n, [&] { return probe_moments_check(e, "rb_probe_moments_device", d_sums, n, d_moments_out); },
        [&](rb_engine* t) { return probe_moments_device_locked(t, d_sums, n, d_moments_out, d_backface_share_out); });
}

int rb_light_points_visible(int32_t device, const rb_probe_grid* grid, const rb_sh9* coeffs, const rb_probe_depth* moments,
                            const rb_surfel* points, size_t m, const rb_light_visibility* params, rb_lit* out) {
    if (const int rc = light_visible_check(nullptr, "rb_light_points_visible", grid, coeffs, moments, points, m, params, out)) return rc;
    if (m == 0) return RB_OK;
    const size_t probes = grid_probes(*grid), piece = std::min(m, light_piece_points());
    rb::DevBuf<rb_sh9> d_coeffs;
    rb::DevBuf<rb_probe_depth> d_moments;
    rb::DevBuf<rb_surfel> d_points;
    rb::DevBuf<rb_lit> d_out;
    DeviceScope s(device);
    s.alloc(d_coeffs, probes);
    if (moments) s.alloc(d_moments, probes);
    s.alloc(d_points, piece);
    s.alloc(d_out, piece);
    s.upload(d_coeffs.ptr, coeffs, probes * sizeof(rb_sh9));   // once per call, like the maps
    if (moments) s.upload(d_moments.ptr, moments, probes * sizeof(rb_probe_depth));
    for (size_t done = 0; done < m && s.ok(); done += piece) {
        const size_t k = std::min(piece, m - done);
        s.upload(d_points.ptr, points + done, k * sizeof(rb_surfel));
        s.run([&] {
            return rb::launch_probe_light_vis(rb::ProbeLightArgs{*grid, d_coeffs.ptr, d_points.ptr, d_out.ptr, static_cast<uint32_t>(k)},
                                              moments ? d_moments.ptr : nullptr, *params, s.stream);
        });
        s.download(out + done, d_out.ptr, k * sizeof(rb_lit));
        s.sync();   // the scratch is the next piece's
    }
    return s.finish("rb_light_points_visible");
}

int rb_light_points_visible_device(rb_engine* e, const rb_probe_grid* grid, const rb_sh9* d_coeffs, const rb_probe_depth* d_moments,
                                   const rb_surfel* d_points, size_t m, const rb_light_visibility* params, rb_lit* d_out) {
    return engine_entry(
        e, m, [&] { return light_visible_check(e, "rb_light_points_visible_device", grid, d_coeffs, d_moments, d_points, m, params, d_out); },
        [&](rb_engine* t) { return light_visible_device_locked(t, *grid, d_coeffs, d_moments, d_points, m, *params, d_out); });
}

int rb_lightmap_surfels(int32_t device, const rb_gpu_triangle* tris, size_t n_tris, const float* uvs, size_t n_uv_floats,
                        const rb_lightmap_params* params, rb_surfel* surfels_out, uint32_t* owners_out) {
    if (!params || !surfels_out || (n_tris > 0 && !tris) || (n_uv_floats > 0 && !uvs))
        return rb::fail(nullptr, RB_ERR_NULL_ARGUMENT, "rb_lightmap_surfels: params / surfels_out / tris / uvs is NULL");
    if (const int rc = lightmap_check(nullptr, "rb_lightmap_surfels", params)) return rc;
    if (n_tris > 0x7FFFFFFFull - 63ull || n_uv_floats > 0xFFFFFFFFull)
        return rb::fail(nullptr, RB_ERR_INVALID_OPTIONS, "rb_lightmap_surfels takes at most 2^31 - 64 triangles and 2^32 - 1 uv floats");
    const size_t n = static_cast<size_t>(params->width) * params->height;
    if (n_tris == 0) {   // nothing covers anything: no device is needed to say so
        std::memset(surfels_out, 0, n * sizeof(rb_surfel));
        if (owners_out) std::memset(owners_out, 0xFF, n * sizeof(uint32_t));
        return RB_OK;
    }
    const uint32_t nt = static_cast<uint32_t>(n_tris), nu = static_cast<uint32_t>(n_uv_floats);
    rb::DevBuf<rb_gpu_triangle> d_tris;
    rb::DevBuf<float> d_uvs;
    rb::DevBuf<uint32_t> d_iota, d_owners;
    rb::DevBuf<rb::PrepTri> d_ptris;
    rb::DevBuf<rb::PrepTriShade> d_pshade;
    rb::DevBuf<unsigned char> d_work;
    rb::DevBuf<rb_surfel> d_surfels;
    DeviceScope s(device);
    s.alloc(d_tris, nt);
    s.alloc(d_uvs, nu);
    s.alloc(d_iota, nt);
    s.alloc(d_ptris, nt);
    s.alloc(d_pshade, nt);
    s.alloc(d_work, rb::lightmap_work_bytes(nt));
    s.alloc(d_owners, n);
    s.alloc(d_surfels, n);
    s.upload(d_tris.ptr, tris, n_tris * sizeof(rb_gpu_triangle));
    s.upload(d_uvs.ptr, uvs, n_uv_floats * sizeof(float));
    s.run([&] {   // every triangle counts as valid: tri_count = n_tris
        return lightmap_generate(*params, d_tris.ptr, nt, nt, d_uvs.ptr, nu, d_iota.ptr, d_ptris.ptr, d_pshade.ptr, d_work.ptr, d_surfels.ptr,
                                 d_owners.ptr, s.stream);
    });
    s.download(surfels_out, d_surfels.ptr, n * sizeof(rb_surfel));
    if (owners_out) s.download(owners_out, d_owners.ptr, n * sizeof(uint32_t));
    return s.finish("rb_lightmap_surfels");
}

int rb_lightmap_surfels_device(rb_engine* e, const rb_lightmap_params* params, rb_surfel* d_surfels, uint32_t* d_owners) {
    return engine_entry(
        e,
        [&] {
            if (!params || !d_surfels) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "rb_lightmap_surfels_device: params / d_surfels is NULL");
            return lightmap_check(e, "rb_lightmap_surfels_device", params);
        },
        [&](rb_engine* t) { return lightmap_surfels_device_locked(t, *params, d_surfels, d_owners); });
}

int rb_lightmap_resolve(int32_t device, uint32_t width, uint32_t height, const rb_radiance* sums, uint32_t dilate, float* rgba_out) {
    if (!sums || !rgba_out) return rb::fail(nullptr, RB_ERR_NULL_ARGUMENT, "rb_lightmap_resolve: sums / rgba_out is NULL");
    if (const int rc = lightmap_size_check(nullptr, "rb_lightmap_resolve", width, height, dilate)) return rc;
    const size_t n = static_cast<size_t>(width) * height;
    rb::DevBuf<rb_radiance> d_sums;
    rb::DevBuf<float> d_out, d_tmp;
    DeviceScope s(device);
    s.alloc(d_sums, n);
    s.alloc(d_out, n * 4);
    if (dilate > 0u) s.alloc(d_tmp, n * 4);
    s.upload(d_sums.ptr, sums, n * sizeof(rb_radiance));
    s.run([&] { return rb::launch_lightmap_resolve(d_sums.ptr, width, height, dilate, d_out.ptr, d_tmp.ptr, s.stream); });
    s.download(rgba_out, d_out.ptr, n * 16);
    return s.finish("rb_lightmap_resolve");
}

int rb_bake_lightmap(rb_engine* e, const rb_lightmap_params* params, uint32_t first_sample, uint32_t samples, float* rgba_out,
                     rb_radiance* sums_out) {
    return bake_lightmap_entry(e, "rb_bake_lightmap", false, params, first_sample, samples, rgba_out, sums_out);
}

int rb_bake_lightmap_device(rb_engine* e, const rb_lightmap_params* params, uint32_t first_sample, uint32_t samples,
                            float* d_rgba_out, rb_radiance* d_sums_out) {
    return bake_lightmap_entry(e, "rb_bake_lightmap_device", true, params, first_sample, samples, d_rgba_out, d_sums_out);
}

int rb_last_lightmap_ms(rb_engine* e, float* surfels_ms, float* resolve_ms) {
    if (!e) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    rb_engine* const t = query_engine(e);
    if (surfels_ms)
        if (const int rc = stage_ms(e, t, t->t_lm_surfels, surfels_ms)) return rc;
    return resolve_ms ? stage_ms(e, t, t->t_lm_resolve, resolve_ms) : RB_OK;
}

int rb_reproject_device(rb_engine* e, const rb_reproject_params* params, uint32_t w, uint32_t h, const rb_view* prev_view, const float* d_prev4,
                        const rb_guide* d_prev_guides, const rb_guide* d_cur_guides, const float* d_cur4, float* d_out4) {
    return engine_entry(
        e, static_cast<size_t>(w) * h,
        [&] { return reproject_check(e, "rb_reproject_device", params, w, h, prev_view, d_prev4, d_prev_guides, d_cur_guides, d_out4); },
        [&](rb_engine* t) { return reproject_device_locked(t, *params, w, h, *prev_view, d_prev4, d_prev_guides, d_cur_guides, d_cur4, d_out4); });
}

const char* rb_last_query_kernel_name(const rb_engine* e) {
    if (!e) return "";
    return rb::is_group(e) ? e->parts[0]->last_query_kernel_name : e->last_query_kernel_name;
}

int rb_last_query_ms(rb_engine* e, float* ms) { return query_stage_ms(e, &rb_engine::t_query, ms); }
int rb_last_camera_rays_ms(rb_engine* e, float* ms) { return query_stage_ms(e, &rb_engine::t_generator, ms); }
int rb_last_probe_project_ms(rb_engine* e, float* ms) { return query_stage_ms(e, &rb_engine::t_sh, ms); }
int rb_last_probe_depth_project_ms(rb_engine* e, float* ms) { return query_stage_ms(e, &rb_engine::t_depth, ms); }

}  // extern "C"
