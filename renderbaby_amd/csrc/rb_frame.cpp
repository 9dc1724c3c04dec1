// rb_frame.cpp -- what an engine does to a finished frame: the edge-avoiding denoiser over the first-hit guide planes and the
// history it can be given across a camera move, with their engine-less forms, their getters and their C entry points (rb_abi.h;
// DESIGN.md sections 13 and 22).  They cast no caller's rays and go through none of the query runners; what they share with
// the queries is rb_queries.hpp's.  (rb_reproject_device is a device query like any other: rb_queries.cpp.)
#include "rb_host_cam.hpp"
#include "rb_queries.hpp"

namespace {

using rb::device_range, rb::DeviceScope, rb::ensure_prepared, rb::frame_piece_rows, rb::page_locked, rb::query_copy_out, rb::reproject_check,
    rb::require_ready, rb::scene_params, rb::stage_ms;

// ---- the denoiser (rb_abi.h).  Like a query it is queued on the engine's stream behind whatever runs
// there, reads the scene and the committed accumulation, and writes buffers of its own.
rb::GuidePlanes guide_planes(rb_engine* e, int set) { return rb::GuidePlanes{e->dn_nt[set].ptr, e->dn_pc[set].ptr, e->dn_al[set].ptr}; }
rb::GuidePlanes guide_planes(rb_engine* e) { return guide_planes(e, e->dn_set); }

int denoise_ready(rb_engine* e) {
    if (rb::is_group(e)) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "the denoiser does not take a multi-device handle: a tap would cross a stripe boundary");
    rb::set_device(e);
    if (e->opt.shard_count > 1) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "the denoiser does not take a sharded engine: a tap would cross a stripe boundary");
    return require_ready(e);
}

// the guide planes of the current scene: the pixel-centre rays through the query kernels straight into device memory, one pack
int ensure_guides(rb_engine* e) {
    e->t_guides.reset();
    if (e->dn_guides_valid) return RB_OK;
    rb::KParams p{};
    int rc = ensure_prepared(e);
    if (!rc) rc = scene_params(e, &p);
    if (rc) return rc;
    const uint32_t w = e->sc.width, h = e->sc.height;
    const size_t n = static_cast<size_t>(w) * h;
    rb::DevBuf<rb_hit> hits;       // the records live until the pack has read them
    rb::DevBuf<rb_surface> surf;
    HIP_TRY(e, hits.resize(n));
    HIP_TRY(e, surf.resize(n));
    if (e->hist_valid && e->hist_set == e->dn_set) e->dn_set ^= 1;   // the history keeps the planes its frame was made with (section 22)
    HIP_TRY(e, e->dn_nt[e->dn_set].resize(n * 4));
    HIP_TRY(e, e->dn_pc[e->dn_set].resize(n * 4));
    HIP_TRY(e, e->dn_al[e->dn_set].resize(n * 4));
    if (n) {
        HIP_TRY(e, e->t_guides.begin(e->stream));
        const uint32_t piece_rows = frame_piece_rows(w);   // as rb_render_hits
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
        HIP_TRY(e, e->t_guides.end(e->stream));
        HIP_TRY(e, hipStreamSynchronize(e->stream));
        float ms = 0.0f;
        HIP_TRY(e, e->t_guides.read(&ms));
    }
    e->dn_guides_valid = true;
    return RB_OK;
}

int denoise_params_check(const rb_engine* e, const rb_denoise_params* prm) {
    const char* why = nullptr;
    if (!rb::denoise_params_valid(*prm, &why)) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "rb_denoise_params: %s", why);
    return RB_OK;
}

int reproject_params_check(const rb_engine* e, const rb_reproject_params* prm) {
    const char* why = nullptr;
    if (!rb::reproject_params_valid(*prm, &why)) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "rb_reproject_params: %s", why);
    return RB_OK;
}

// the view of a render camera (rb_abi.h): rb_host_cam.hpp's steps, then one operation per scalar
rb_view view_of(const rb_camera& cam, uint32_t w, uint32_t h) {
    const rb::CamBasis b = rb::host_cam_basis(cam, w, h);
    rb_view v{};
    for (int k = 0; k < 3; k++) v.pos[k] = cam.pos[k], v.right[k] = b.right[k], v.up[k] = b.up[k], v.fwd[k] = b.fwd[k];
    v.cx = b.wm1 * 0.5f;
    v.cy = b.hm1 * 0.5f;
    const float fa = b.fov * b.aspect;
    v.sx = v.cx / fa;
    v.sy = v.cy / b.fov;
    return v;
}

// Steps 2 to 4 of rb_denoise_history (section 22.2) on the engine's stream; the guides are current.  Afterwards e->hist_frame
// holds F.
int history_step(rb_engine* e, const rb_reproject_params& prm) {
    const uint32_t w = e->sc.width, h = e->sc.height;
    const size_t n = static_cast<size_t>(w) * h;
    e->t_history.reset();
    HIP_TRY(e, e->hist_base.resize(n * 4));
    // (an accepted update stands between H and an invalid base, and ensure_guides has built its guides into the other set)
    const bool carry = !e->hist_base_valid && e->hist_valid && e->hist_w == w && e->hist_h == h && rb::view_finite(e->hist_view) &&
                       e->hist_set != e->dn_set;
    if (!e->hist_base_valid && !carry) {
        e->hist_valid = false;
        HIP_TRY(e, e->hist_frame.resize(n * 4));
    }
    HIP_TRY(e, e->t_history.begin(e->stream));
    if (!e->hist_base_valid) {
        if (carry) {
            rb::ReprojectArgs a{};
            a.w = w;
            a.h = h;
            a.view = e->hist_view;
            a.prev4 = e->hist_frame.ptr;
            a.prev = guide_planes(e, e->hist_set);
            a.cur = guide_planes(e);
            a.out4 = e->hist_base.ptr;
            const int st = rb::launch_reproject(prm, a, e->stream);
            if (st) return rb::fail(e, RB_ERR_DEVICE, "reproject kernel launch failed: %s", hipGetErrorString(static_cast<hipError_t>(st)));
        } else {
            HIP_TRY(e, hipMemsetAsync(e->hist_base.ptr, 0, n * 16, e->stream));   // every record NONE
        }
        e->hist_set = e->dn_set;   // the history's guides from here on: this update's planes, shared with the filter
        e->hist_view = view_of(e->sc.uniforms.camera, w, h);
        e->hist_w = w;
        e->hist_h = h;
        e->hist_base_valid = true;
    }
    const int st = rb::launch_history_merge(w, h, e->slot[e->cur].accum.ptr, e->hist_base.ptr, guide_planes(e), e->hist_frame.ptr, e->stream);
    if (st) return rb::fail(e, RB_ERR_DEVICE, "history merge launch failed: %s", hipGetErrorString(static_cast<hipError_t>(st)));
    HIP_TRY(e, e->t_history.end(e->stream));
    e->hist_valid = true;
    return RB_OK;
}

// device == true: the outputs are the caller's device buffers and nothing is waited for.  rprm: rb_denoise_history -- the filter
// runs on F of section 22 instead of the mean radiance
int denoise_locked(rb_engine* e, const rb_denoise_params* prm, uint8_t* rgba_out, float* linear_out, bool device,
                   const rb_reproject_params* rprm = nullptr) {
    int rc = denoise_ready(e);
    if (!rc) rc = denoise_params_check(e, prm);
    if (!rc && rprm) rc = reproject_params_check(e, rprm);
    if (rc) return rc;
    if (!rgba_out && !linear_out) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "rgba_out and linear_out are both NULL");
    const size_t n = static_cast<size_t>(e->sc.width) * e->sc.height;
    if (device) {
        if (rgba_out) rc = device_range(e, rgba_out, n * 4, 4, "d_rgba_out");
        if (!rc && linear_out) rc = device_range(e, linear_out, n * 16, 16, "d_linear_out");
        if (rc) return rc;
    }
    rc = ensure_guides(e);
    if (rc) return rc;
    e->t_filter.reset();
    if (n == 0) return RB_OK;
    rb::DenoiseArgs a{};
    a.w = e->sc.width;
    a.h = e->sc.height;
    a.accum = e->slot[e->cur].accum.ptr;
    a.g = guide_planes(e);
    for (int k = 0; k < 2; ++k) {
        HIP_TRY(e, e->dn_r[k].resize(n * 4));
        a.r[k] = e->dn_r[k].ptr;
    }
    if (!device) {   // (reserved before the history moves: a failed reservation leaves H as it was)
        if (rgba_out) HIP_TRY(e, e->dn_rgba.resize(n));
        if (linear_out) HIP_TRY(e, e->dn_linear.resize(n * 4));
    }
    if (rprm) {
        rc = history_step(e, *rprm);
        if (rc) return rc;
        a.accum = nullptr;
        a.color4 = e->hist_frame.ptr;
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
    HIP_TRY(e, e->t_filter.begin(e->stream));
    const int st = rb::launch_denoise(*prm, a, e->stream);
    if (st) return rb::fail(e, RB_ERR_DEVICE, "denoise kernel launch failed: %s", hipGetErrorString(static_cast<hipError_t>(st)));
    HIP_TRY(e, e->t_filter.end(e->stream));
    if (device) return RB_OK;   // rb_last_denoise_ms reads the pair when it is asked
    if (rgba_out) rc = query_copy_out(e, rgba_out, e->dn_rgba.ptr, n * 4, page_locked(rgba_out));
    if (!rc && linear_out) rc = query_copy_out(e, linear_out, e->dn_linear.ptr, n * 16, page_locked(linear_out));
    if (rc) return rc;
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return RB_OK;
}

int denoise_guides_locked(rb_engine* e, rb_guide* guides_out) {
    int rc = denoise_ready(e);
    if (!rc) rc = ensure_guides(e);
    if (rc) return rc;
    const size_t n = static_cast<size_t>(e->sc.width) * e->sc.height;
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

int history_read_locked(rb_engine* e, float* out4) {
    int rc = denoise_ready(e);
    if (rc) return rc;
    if (!e->hist_valid || e->hist_w != e->sc.width || e->hist_h != e->sc.height)   // (a history of another size is none: out4 is the current frame's)
        return rb::fail(e, RB_ERR_NOT_INITIALIZED, "rb_history_read: the engine has no history of this size (rb_denoise_history makes it)");
    const size_t n = static_cast<size_t>(e->hist_w) * e->hist_h;
    if (n == 0) return RB_OK;
    rc = query_copy_out(e, out4, e->hist_frame.ptr, n * 16, page_locked(out4));
    if (rc) return rc;
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return RB_OK;
}

}  // namespace

// ---- temporal reprojection (rb_abi.h)
// the refusals the forms of rb_reproject share; before a device is touched (e may be NULL: the engine-less form)
int rb::reproject_check(rb_engine* e, const char* who, const rb_reproject_params* prm, uint32_t w, uint32_t h, const rb_view* view, const void* prev4,
                    const void* prev_guides, const void* cur_guides, const void* out4) {
    if (!prm || !view || !prev4 || !prev_guides || !cur_guides || !out4)
        return rb::fail(e, RB_ERR_NULL_ARGUMENT, "%s: params / prev_view / prev4 / prev_guides / cur_guides / out4 is NULL", who);
    if (const int rc = reproject_params_check(e, prm)) return rc;
    if (!rb::view_finite(*view)) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: a word of prev_view is not finite", who);
    if (static_cast<uint64_t>(w) * h >= (1ull << 31)) return rb::fail(e, RB_ERR_INVALID_OPTIONS, "%s: a frame of %u x %u pixels is too large", who, w, h);
    return RB_OK;
}

extern "C" {

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
    if (const int rc = stage_ms(e, e, e->t_filter, ms)) return rc;   // (rb_denoise_device returned without waiting)
    return guide_build_ms ? stage_ms(e, e, e->t_guides, guide_build_ms) : RB_OK;
}

int rb_denoise_buffers(int32_t device, const rb_denoise_params* params, uint32_t w, uint32_t h, const float* color4,
                       const rb_guide* guides, float* out4, uint8_t* rgba_out) {
    if (!params || !color4 || !guides) return rb::fail(nullptr, RB_ERR_NULL_ARGUMENT, "params / color4 / guides is NULL");
    if (!out4 && !rgba_out) return rb::fail(nullptr, RB_ERR_NULL_ARGUMENT, "out4 and rgba_out are both NULL");
    if (const int rc = denoise_params_check(nullptr, params)) return rc;
    const size_t n = static_cast<size_t>(w) * h;
    if (n >= (1ull << 31)) return rb::fail(nullptr, RB_ERR_INVALID_OPTIONS, "a frame of %u x %u pixels is too large", w, h);
    if (n == 0) return RB_OK;
    rb::DevBuf<float> d_color, d_nt, d_pc, d_al, d_r0, d_r1, d_linear;
    rb::DevBuf<rb_guide> d_guides;
    rb::DevBuf<uint32_t> d_rgba;
    DeviceScope s(device);
    for (rb::DevBuf<float>* b : {&d_color, &d_nt, &d_pc, &d_al, &d_r0, &d_r1}) s.alloc(*b, n * 4);
    s.alloc(d_guides, n);
    if (out4) s.alloc(d_linear, n * 4);
    if (rgba_out) s.alloc(d_rgba, n);
    s.upload(d_color.ptr, color4, n * 16);
    s.upload(d_guides.ptr, guides, n * sizeof(rb_guide));
    rb::DenoiseArgs a{};
    a.w = w;
    a.h = h;
    a.color4 = d_color.ptr;
    a.g = rb::GuidePlanes{d_nt.ptr, d_pc.ptr, d_al.ptr};
    a.r[0] = d_r0.ptr;
    a.r[1] = d_r1.ptr;
    a.linear_out = d_linear.ptr;
    a.rgba_out = d_rgba.ptr;
    s.run([&] { return rb::launch_guide_split(d_guides.ptr, n, a.g, s.stream); });
    s.run([&] { return rb::launch_denoise(*params, a, s.stream); });
    if (out4) s.download(out4, d_linear.ptr, n * 16);
    if (rgba_out) s.download(rgba_out, d_rgba.ptr, n * 4);
    return s.finish("rb_denoise_buffers");
}

int rb_view_from_camera(const rb_camera* cam, uint32_t w, uint32_t h, rb_view* out) {
    if (!cam || !out) return rb::fail(nullptr, RB_ERR_NULL_ARGUMENT, "rb_view_from_camera: cam / out is NULL");
    *out = view_of(*cam, w, h);
    return RB_OK;
}

int rb_reproject_default_params(rb_reproject_params* p) {
    if (!p) return RB_ERR_NULL_ARGUMENT;
    *p = rb_reproject_params{};
    p->sigma_depth = 0.02f;    // the denoiser's plane distance and floor (section 13)
    p->normal_min = 0.9f;      // from the literature, or the sweep of DESIGN.md section 22.5: section 22.7 says which
    p->albedo_floor = 0.01f;
    p->max_history = 32.0f;
    return RB_OK;
}

int rb_reproject_buffers(int32_t device, const rb_reproject_params* params, uint32_t w, uint32_t h, const rb_view* prev_view,
                         const float* prev4, const rb_guide* prev_guides, const rb_guide* cur_guides, const float* cur4, float* out4) {
    if (const int rc = reproject_check(nullptr, "rb_reproject_buffers", params, w, h, prev_view, prev4, prev_guides, cur_guides, out4)) return rc;
    const size_t n = static_cast<size_t>(w) * h;
    if (n == 0) return RB_OK;
    rb::DevBuf<float> d_prev4, d_cur4, d_out, d_pl[6];
    rb::DevBuf<rb_guide> d_guides;   // staging of one guide array at a time
    DeviceScope s(device);
    s.alloc(d_prev4, n * 4);
    if (cur4) s.alloc(d_cur4, n * 4);
    s.alloc(d_out, n * 4);
    for (rb::DevBuf<float>& b : d_pl) s.alloc(b, n * 4);
    s.alloc(d_guides, n);
    rb::ReprojectArgs a{};
    a.w = w;
    a.h = h;
    a.view = *prev_view;
    a.prev4 = d_prev4.ptr;
    a.prev = rb::GuidePlanes{d_pl[0].ptr, d_pl[1].ptr, d_pl[2].ptr};
    a.cur = rb::GuidePlanes{d_pl[3].ptr, d_pl[4].ptr, d_pl[5].ptr};
    a.cur4 = cur4 ? d_cur4.ptr : nullptr;
    a.out4 = d_out.ptr;
    s.upload(d_prev4.ptr, prev4, n * 16);
    if (cur4) s.upload(d_cur4.ptr, cur4, n * 16);
    s.upload(d_guides.ptr, prev_guides, n * sizeof(rb_guide));
    s.run([&] { return rb::launch_guide_split(d_guides.ptr, n, a.prev, s.stream); });
    s.upload(d_guides.ptr, cur_guides, n * sizeof(rb_guide));   // (in stream order behind the split that read the staging)
    s.run([&] { return rb::launch_guide_split(d_guides.ptr, n, a.cur, s.stream); });
    s.run([&] { return rb::launch_reproject(*params, a, s.stream); });
    s.download(out4, d_out.ptr, n * 16);
    return s.finish("rb_reproject_buffers");
}

int rb_denoise_history(rb_engine* e, const rb_reproject_params* rparams, const rb_denoise_params* dparams, uint8_t* rgba_out, float* linear_out) {
    if (!e || !rparams || !dparams) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    return denoise_locked(e, dparams, rgba_out, linear_out, false, rparams);
}

int rb_denoise_history_device(rb_engine* e, const rb_reproject_params* rparams, const rb_denoise_params* dparams, uint8_t* d_rgba_out,
                              float* d_linear_out) {
    if (!e || !rparams || !dparams) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    return denoise_locked(e, dparams, d_rgba_out, d_linear_out, true, rparams);
}

int rb_history_read(rb_engine* e, float* out4) {
    if (!e) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    if (!out4) return rb::fail(e, RB_ERR_NULL_ARGUMENT, "out4 is NULL");
    return history_read_locked(e, out4);
}

int rb_history_reset(rb_engine* e) {
    if (!e) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    if (rb::is_group(e)) return RB_OK;   // a multi-device handle keeps no history
    e->hist_valid = false;
    e->hist_base_valid = false;
    return RB_OK;
}

int rb_last_reproject_ms(rb_engine* e, float* ms) {
    if (!e || !ms) return RB_ERR_NULL_ARGUMENT;
    std::lock_guard<std::mutex> lock(e->mu);
    return stage_ms(e, e, e->t_history, ms);   // (the history step is not waited for)
}

}  // extern "C"
