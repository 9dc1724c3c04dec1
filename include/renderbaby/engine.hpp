// engine.hpp -- C++ host-side mirror of the reference's renderer interface over
// the C ABI (rb_abi.h).  Header-only; the reference's toolchain (Rust) is absent
// from this image, so this is the compiled-language host layer a C++ caller uses
// and the template for the Rust shim in INTEGRATION.md.
//
//   Change<T>, RenderConfig        crates/engine-config/src/render_config.rs:37-57,99-109
//   trait Renderer                 crates/engine-config/src/renderer.rs:35-66
//   Engine::new / render / frame_iterator
//                                  crates/engine-pathtracer/src/lib.rs:58-119
//   Frame, trait FrameIterator     crates/frame-buffer/src/frame_iterator.rs:3-51
//
// Errors are exceptions carrying the rb_abi.h status and the library's message
// (the reference returns anyhow::Error or panics).
#pragma once

#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../rb_abi.h"

namespace renderbaby {

struct RenderError : std::runtime_error {
    int code;
    RenderError(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

// enum Change<T> { Keep, Create(T), Update(T), Delete }
template <typename T>
struct Change {
    uint32_t tag = RB_KEEP;
    T value{};
    static Change keep() { return {}; }
    static Change create(T v) { return {RB_CREATE, std::move(v)}; }
    static Change update(T v) { return {RB_UPDATE, std::move(v)}; }
    static Change remove() { Change c; c.tag = RB_DELETE; return c; }
};

struct TextureData {  // crates/engine-config/src/texture.rs:26-36
    uint32_t width = 0, height = 0;
    std::vector<uint32_t> rgba_data;
};

struct RenderConfig {
    Change<rb_uniforms> uniforms;
    Change<std::vector<rb_sphere>> spheres;
    Change<std::vector<float>> uvs;
    Change<std::vector<rb_mesh>> meshes;
    Change<std::vector<rb_point_light>> lights;
    Change<std::vector<rb_bvh_node>> bvh_nodes;
    Change<std::vector<uint32_t>> bvh_indices;
    Change<std::vector<rb_gpu_triangle>> bvh_triangles;
    Change<std::vector<TextureData>> textures;
};

// struct Frame { width, height, pixels: Vec<u8> } -- RGBA8, x mirrored, A = 255
struct Frame {
    size_t width = 0, height = 0;
    std::vector<uint8_t> pixels;
    size_t expected_size() const { return width * height * 4; }
    void validate() const {
        if (pixels.size() != expected_size())
            throw RenderError(0, "Frame pixel size mismatch: expected " + std::to_string(expected_size()) +
                                     " bytes, got " + std::to_string(pixels.size()));
    }
};

// trait FrameIterator: Send + 'static { has_next, next, destroy }
struct FrameIterator {
    virtual ~FrameIterator() = default;
    virtual bool has_next() const = 0;
    virtual Frame next() = 0;
    virtual void destroy() = 0;
};

// trait Renderer: Send { render, frame_iterator }
struct Renderer {
    virtual ~Renderer() = default;
    virtual Frame render(const RenderConfig& rc) = 0;
    virtual std::unique_ptr<FrameIterator> frame_iterator(const RenderConfig& rc) = 0;
};

namespace detail {
// Borrowed view of a RenderConfig as rb_config; lives for one call.
struct Marshal {
    rb_config c{};
    std::vector<rb_texture> tex;
    explicit Marshal(const RenderConfig& rc) {
        c.uniforms = {rc.uniforms.tag, &rc.uniforms.value, 1};
        if (rc.uniforms.tag == RB_KEEP || rc.uniforms.tag == RB_DELETE) c.uniforms = {rc.uniforms.tag, nullptr, 0};
        auto vec = [](auto& ch) { return rb_field{ch.tag, ch.value.empty() ? nullptr : ch.value.data(), ch.value.size()}; };
        c.spheres = vec(rc.spheres);
        c.uvs = vec(rc.uvs);
        c.meshes = vec(rc.meshes);
        c.lights = vec(rc.lights);
        c.bvh_nodes = vec(rc.bvh_nodes);
        c.bvh_indices = vec(rc.bvh_indices);
        c.bvh_triangles = vec(rc.bvh_triangles);
        for (const auto& t : rc.textures.value) tex.push_back(rb_texture{t.width, t.height, t.rgba_data.data()});
        c.textures = {rc.textures.tag, tex.empty() ? nullptr : tex.data(), tex.size()};
    }
};
}  // namespace detail

// engine_pathtracer::Engine for the HIP backend.  Like the reference's
// Arc<Mutex<GpuWrapper>>, the handle is shared with the iterator and every call is
// serialised inside the library; Engine is safe to move across threads.
class Engine final : public Renderer {
    struct Handle {
        rb_engine* e;
        explicit Handle(rb_engine* p) : e(p) {}
        ~Handle() { rb_destroy(e); }
    };
    std::shared_ptr<Handle> h_;

    static void check(rb_engine* e, int rc) {
        if (rc != RB_OK) throw RenderError(rc, rb_last_error(e));
    }
    static Frame make_frame(rb_engine* e) {
        uint32_t w = 0, h = 0;
        check(e, rb_get_size(e, &w, &h));
        Frame f;
        f.width = w;
        f.height = h;
        f.pixels.resize(static_cast<size_t>(w) * h * 4);
        return f;
    }

    class Iter final : public FrameIterator {
        std::shared_ptr<Handle> h_;
      public:
        explicit Iter(std::shared_ptr<Handle> h) : h_(std::move(h)) {}
        bool has_next() const override { return rb_iter_has_next(h_->e) != 0; }
        Frame next() override {
            if (!has_next()) throw RenderError(RB_ERR_NO_MORE_FRAMES, "No more frames available");
            Frame f = make_frame(h_->e);
            check(h_->e, rb_iter_next(h_->e, f.pixels.data()));
            return f;
        }
        void destroy() override { rb_iter_destroy(h_->e); }
    };
    // extension: one frame per `n` samples instead of per sample (rb_iter_set_passes_per_frame)
  public:
    void set_passes_per_frame(uint32_t n) { check(h_->e, rb_iter_set_passes_per_frame(h_->e, n)); }
  private:

  public:
    // Engine::new(rc)
    explicit Engine(const RenderConfig& rc, const rb_options* opt = nullptr) {
        detail::Marshal m(rc);
        rb_engine* e = rb_create_ex(&m.c, opt);
        if (!e) throw RenderError(RB_ERR_DEVICE, rb_last_error(nullptr));
        h_ = std::make_shared<Handle>(e);
    }
    Frame render(const RenderConfig& rc) override {
        detail::Marshal m(rc);
        check(h_->e, rb_update(h_->e, &m.c));
        Frame f = make_frame(h_->e);
        check(h_->e, rb_render(h_->e, f.pixels.data()));
        return f;
    }
    std::unique_ptr<FrameIterator> frame_iterator(const RenderConfig& rc) override {
        detail::Marshal m(rc);
        check(h_->e, rb_iter_begin(h_->e, &m.c));
        return std::make_unique<Iter>(h_);
    }
    // ---- closest-hit queries (extension; rb_abi.h): what closest_hit holds for a ray, without shading
    struct Hits {
        uint32_t width = 0, rows = 0;       // rows: the image height (a sharded engine: its padded local rows)
        std::vector<rb_hit> hits;           // [row * width + x], orientation of the delivered frame
        std::vector<rb_surface> surfaces;   // empty unless asked for
    };
    Hits cast_rays(const std::vector<rb_ray>& rays, bool surfaces = false) {
        Hits r;
        r.width = static_cast<uint32_t>(rays.size());
        r.rows = 1;
        r.hits.resize(rays.size());
        if (surfaces) r.surfaces.resize(rays.size());
        check(h_->e, rb_cast_rays(h_->e, rays.data(), rays.size(), r.hits.data(), surfaces ? r.surfaces.data() : nullptr));
        return r;
    }
    Hits render_hits(bool surfaces = false) {
        Hits r;
        uint32_t h = 0, owned = 0, padded = 0;
        check(h_->e, rb_get_size(h_->e, &r.width, &h));
        check(h_->e, rb_local_rows(h_->e, &owned, &padded));
        r.rows = padded;   // == height unless sharded
        r.hits.resize(static_cast<size_t>(r.width) * r.rows);
        if (surfaces) r.surfaces.resize(r.hits.size());
        check(h_->e, rb_render_hits(h_->e, r.hits.data(), surfaces ? r.surfaces.data() : nullptr));
        return r;
    }
    // ---- any-hit occlusion and device-resident buffers (extension; rb_abi.h)
    // RB_OCCL_* per ray: is anything within (0.001, tmax) among the stages of `mask`?  tmax: empty (no bound) or one per ray
    std::vector<uint8_t> occluded(const std::vector<rb_ray>& rays, const std::vector<float>& tmax = {}, uint32_t mask = RB_MASK_ALL) {
        if (!tmax.empty() && tmax.size() != rays.size()) throw std::invalid_argument("rays and tmax differ in length");
        std::vector<uint8_t> out(rays.size());
        check(h_->e, rb_occluded(h_->e, rays.data(), tmax.empty() ? nullptr : tmax.data(), rays.size(), mask, out.data()));
        return out;
    }
    // the same on buffers in the engine's device memory: queued on the engine's stream, no copy; sync() is the wait
    void occluded_device(const rb_ray* d_rays, const float* d_tmax, size_t n, uint8_t* d_out, uint32_t mask = RB_MASK_ALL) {
        check(h_->e, rb_occluded_device(h_->e, d_rays, d_tmax, n, mask, d_out));
    }
    void cast_rays_device(const rb_ray* d_rays, size_t n, rb_hit* d_hits, rb_surface* d_surf = nullptr) {
        check(h_->e, rb_cast_rays_device(h_->e, d_rays, n, d_hits, d_surf));
    }
    // ---- path-traced radiance along given rays (extension; rb_abi.h): per ray the ordered sum of
    // `samples` evaluations of trace_ray and the weight; seeds: empty (the ray's index) or one id per ray
    std::vector<rb_radiance> trace_rays(const std::vector<rb_ray>& rays, const std::vector<uint32_t>& seeds = {}, uint32_t samples = 1,
                                        uint32_t first_sample = 0) {
        if (!seeds.empty() && seeds.size() != rays.size()) throw std::invalid_argument("rays and seeds differ in length");
        std::vector<rb_radiance> out(rays.size());
        check(h_->e, rb_trace_rays(h_->e, rays.data(), seeds.empty() ? nullptr : seeds.data(), rays.size(), first_sample, samples, out.data()));
        return out;
    }
    // the same on buffers in the engine's device memory: queued on the engine's stream, not waited for -- sync() waits
    void trace_rays_device(const rb_ray* d_rays, const uint32_t* d_seeds, size_t n, rb_radiance* d_out, uint32_t samples = 1,
                           uint32_t first_sample = 0) {
        check(h_->e, rb_trace_rays_device(h_->e, d_rays, d_seeds, n, first_sample, samples, d_out));
    }
    // ---- camera rays made on the device (extension; rb_abi.h): per pixel of [first_pixel, first_pixel +
    // n_pixels) the ordered sum over `samples` rays, each made from its own random stream; n_pixels = 0: the whole image
    std::vector<rb_radiance> trace_camera(const rb_camera_ex& cam, uint32_t samples, uint32_t first_sample = 0, uint64_t first_pixel = 0,
                                          size_t n_pixels = 0) {
        if (n_pixels == 0 && first_pixel == 0) n_pixels = static_cast<size_t>(cam.width) * cam.height;
        std::vector<rb_radiance> out(n_pixels);
        check(h_->e, rb_trace_camera(h_->e, &cam, first_pixel, n_pixels, first_sample, samples, out.data()));
        return out;
    }
    // the same into the engine's device memory: queued on the engine's stream, not waited for -- sync() waits
    void trace_camera_device(const rb_camera_ex& cam, uint64_t first_pixel, size_t n_pixels, rb_radiance* d_out, uint32_t samples,
                             uint32_t first_sample = 0) {
        check(h_->e, rb_trace_camera_device(h_->e, &cam, first_pixel, n_pixels, first_sample, samples, d_out));
    }
    // ---- hemisphere rays made on the device (extension; rb_abi.h): per surfel the ordered sum over
    // `samples` cosine-weighted rays about its normal, or the count of those that meet nothing within `radius`
    static rb_hemi_params hemi_params(float offset = 1e-3f, float radius = 0.0f, uint32_t mask = 0) {
        rb_hemi_params p{};
        p.offset = offset;
        p.radius = radius;
        p.mask = mask;
        return p;
    }
    std::vector<rb_radiance> trace_hemisphere(const std::vector<rb_surfel>& surfels, uint32_t samples, uint32_t first_sample = 0,
                                              const uint32_t* seeds = nullptr, float offset = 1e-3f) {
        const rb_hemi_params p = hemi_params(offset);
        std::vector<rb_radiance> out(surfels.size());
        check(h_->e, rb_trace_hemisphere(h_->e, surfels.data(), seeds, surfels.size(), &p, first_sample, samples, out.data()));
        return out;
    }
    std::vector<rb_openness> openness(const std::vector<rb_surfel>& surfels, uint32_t samples, float radius,
                                      uint32_t mask = RB_MASK_ALL & ~RB_MASK_LIGHTS, uint32_t first_sample = 0,
                                      const uint32_t* seeds = nullptr, float offset = 1e-3f) {
        const rb_hemi_params p = hemi_params(offset, radius, mask);
        std::vector<rb_openness> out(surfels.size());
        check(h_->e, rb_openness_hemisphere(h_->e, surfels.data(), seeds, surfels.size(), &p, first_sample, samples, out.data()));
        return out;
    }
    // the same on the engine's device memory: queued on the engine's stream, not waited for -- sync() waits
    void trace_hemisphere_device(const rb_surfel* d_surfels, const uint32_t* d_seeds, size_t n, const rb_hemi_params& p, rb_radiance* d_out,
                                 uint32_t samples, uint32_t first_sample = 0) {
        check(h_->e, rb_trace_hemisphere_device(h_->e, d_surfels, d_seeds, n, &p, first_sample, samples, d_out));
    }
    void openness_device(const rb_surfel* d_surfels, const uint32_t* d_seeds, size_t n, const rb_hemi_params& p, rb_openness* d_out,
                         uint32_t samples, uint32_t first_sample = 0) {
        check(h_->e, rb_openness_hemisphere_device(h_->e, d_surfels, d_seeds, n, &p, first_sample, samples, d_out));
    }
    // ---- direct light at surface points (extension; rb_abi.h): the scene's emitter table, and per surfel
    // the ordered sum over `samples` shadow rays towards points drawn on its emitters (an empty `emitters`: the scene's own)
    static rb_light_params light_params(float offset = 1e-3f, float shorten = 1e-3f, uint32_t mask = RB_MASK_ALL) {
        rb_light_params p{};
        p.offset = offset;
        p.shorten = shorten;
        p.mask = mask;
        return p;
    }
    std::vector<rb_emitter> scene_emitters() {
        size_t count = 0;
        check(h_->e, rb_scene_emitters(h_->e, nullptr, 0, &count));
        std::vector<rb_emitter> out(count);
        check(h_->e, rb_scene_emitters(h_->e, out.data(), out.size(), &count));
        return out;
    }
    std::vector<rb_radiance> direct_light(const std::vector<rb_surfel>& surfels, uint32_t samples, uint32_t first_sample = 0,
                                          const uint32_t* seeds = nullptr, const rb_light_params& p = light_params(),
                                          const std::vector<rb_emitter>& emitters = {}) {
        std::vector<rb_radiance> out(surfels.size());
        check(h_->e, rb_direct_light(h_->e, emitters.empty() ? nullptr : emitters.data(), emitters.size(), surfels.data(), seeds, surfels.size(), &p,
                                     first_sample, samples, out.data()));
        return out;
    }
    // the same on the engine's device memory (d_emitters == nullptr: the scene's own table): queued, not waited for -- sync() waits
    void scene_emitters_device(rb_emitter* d_out, size_t capacity, uint32_t* d_count) {
        check(h_->e, rb_scene_emitters_device(h_->e, d_out, capacity, d_count));
    }
    void direct_light_device(const rb_emitter* d_emitters, size_t n_emit, const rb_surfel* d_surfels, const uint32_t* d_seeds, size_t n,
                             const rb_light_params& p, rb_radiance* d_out, uint32_t samples, uint32_t first_sample = 0) {
        check(h_->e, rb_direct_light_device(h_->e, d_emitters, n_emit, d_surfels, d_seeds, n, &p, first_sample, samples, d_out));
    }
    // ---- ... with a weighted pick (extension; rb_abi.h): the scene's table of pick weights by power, and
    // direct_light with the emitters picked by it -- or, for a table of the caller's, by `cdf` (one inclusive weight per emitter;
    // empty: by the power of those emitters)
    std::vector<uint32_t> scene_emitter_cdf() {
        size_t count = 0;
        check(h_->e, rb_scene_emitter_cdf(h_->e, nullptr, 0, &count));
        std::vector<uint32_t> out(count);
        check(h_->e, rb_scene_emitter_cdf(h_->e, out.data(), out.size(), &count));
        return out;
    }
    std::vector<rb_radiance> direct_light_cdf(const std::vector<rb_surfel>& surfels, uint32_t samples, uint32_t first_sample = 0,
                                              const uint32_t* seeds = nullptr, const rb_light_params& p = light_params(),
                                              const std::vector<rb_emitter>& emitters = {}, const std::vector<uint32_t>& cdf = {}) {
        if (!cdf.empty() && cdf.size() != emitters.size()) throw std::invalid_argument("direct_light_cdf: one cdf entry per emitter is needed");
        std::vector<rb_radiance> out(surfels.size());
        check(h_->e, rb_direct_light_cdf(h_->e, emitters.empty() ? nullptr : emitters.data(), cdf.empty() ? nullptr : cdf.data(), emitters.size(),
                                         surfels.data(), seeds, surfels.size(), &p, first_sample, samples, out.data()));
        return out;
    }
    // the table by power of a caller's emitters, no engine, made on `device` (-1: the current one)
    static std::vector<uint32_t> emitter_cdf(const std::vector<rb_emitter>& emitters, int32_t device = -1) {
        std::vector<uint32_t> out(emitters.size());
        check(nullptr, rb_emitter_cdf(device, emitters.data(), emitters.size(), out.data()));
        return out;
    }
    void scene_emitter_cdf_device(uint32_t* d_out, size_t capacity, uint32_t* d_count) {
        check(h_->e, rb_scene_emitter_cdf_device(h_->e, d_out, capacity, d_count));
    }
    void direct_light_cdf_device(const rb_emitter* d_emitters, const uint32_t* d_cdf, size_t n_emit, const rb_surfel* d_surfels,
                                 const uint32_t* d_seeds, size_t n, const rb_light_params& p, rb_radiance* d_out, uint32_t samples,
                                 uint32_t first_sample = 0) {
        check(h_->e, rb_direct_light_cdf_device(h_->e, d_emitters, d_cdf, n_emit, d_surfels, d_seeds, n, &p, first_sample, samples, d_out));
    }
    // ---- ... with the emitters picked per grid cell (extension; rb_abi.h): one table of pick weights per
    // cell of `grid` (its counts count cells), nx * ny * nz rows of one entry per emitter; `tables` empty: made for the call
    static std::vector<uint32_t> emitter_grid_cdf(const std::vector<rb_emitter>& emitters, const rb_probe_grid& grid, int32_t device = -1) {
        std::vector<uint32_t> out(emitters.size() * grid.counts[0] * grid.counts[1] * grid.counts[2]);
        check(nullptr, rb_emitter_grid_cdf(device, emitters.data(), emitters.size(), &grid, out.data()));
        return out;
    }
    // d_emitters == nullptr: the scene's table, n_emit its count (scene_emitters().size())
    void emitter_grid_cdf_device(const rb_emitter* d_emitters, size_t n_emit, const rb_probe_grid& grid, uint32_t* d_tables_out) {
        check(h_->e, rb_emitter_grid_cdf_device(h_->e, d_emitters, n_emit, &grid, d_tables_out));
    }
    // `emitters` empty: the scene's table, of `scene_count` records (scene_emitters().size())
    std::vector<rb_radiance> direct_light_grid(const std::vector<rb_surfel>& surfels, const rb_probe_grid& grid, uint32_t samples,
                                               size_t scene_count = 0, uint32_t first_sample = 0, const uint32_t* seeds = nullptr,
                                               const rb_light_params& p = light_params(), const std::vector<rb_emitter>& emitters = {},
                                               const std::vector<uint32_t>& tables = {}) {
        const size_t n_emit = emitters.empty() ? scene_count : emitters.size();
        if (!tables.empty() && tables.size() != n_emit * grid.counts[0] * grid.counts[1] * grid.counts[2])
            throw std::invalid_argument("direct_light_grid: one entry per cell and emitter is needed");
        std::vector<rb_radiance> out(surfels.size());
        check(h_->e, rb_direct_light_grid(h_->e, emitters.empty() ? nullptr : emitters.data(), &grid, tables.empty() ? nullptr : tables.data(),
                                          n_emit, surfels.data(), seeds, surfels.size(), &p, first_sample, samples, out.data()));
        return out;
    }
    void direct_light_grid_device(const rb_emitter* d_emitters, const rb_probe_grid& grid, const uint32_t* d_tables, size_t n_emit,
                                  const rb_surfel* d_surfels, const uint32_t* d_seeds, size_t n, const rb_light_params& p, rb_radiance* d_out,
                                  uint32_t samples, uint32_t first_sample = 0) {
        check(h_->e, rb_direct_light_grid_device(h_->e, d_emitters, &grid, d_tables, n_emit, d_surfels, d_seeds, n, &p, first_sample, samples, d_out));
    }
    // ---- ... and tables that learn visibility (extension; rb_abi.h): `tally` holds one record per cell and
    // emitter, which the call adds its shadow rays to (the caller zeroes it and keeps it); `sums` false: a training-only call
    std::vector<rb_radiance> direct_light_grid_tally(const std::vector<rb_surfel>& surfels, const rb_probe_grid& grid, uint32_t samples,
                                                     std::vector<rb_grid_tally>& tally, size_t scene_count = 0, uint32_t first_sample = 0,
                                                     const uint32_t* seeds = nullptr, const rb_light_params& p = light_params(),
                                                     const std::vector<rb_emitter>& emitters = {}, const std::vector<uint32_t>& tables = {},
                                                     bool sums = true) {
        const size_t n_emit = emitters.empty() ? scene_count : emitters.size();
        const size_t entries = n_emit * grid.counts[0] * grid.counts[1] * grid.counts[2];
        if (tally.size() != entries || (!tables.empty() && tables.size() != entries))
            throw std::invalid_argument("direct_light_grid_tally: one entry per cell and emitter is needed");
        std::vector<rb_radiance> out(sums ? surfels.size() : 0);
        rb_grid_tally none{};
        check(h_->e, rb_direct_light_grid_tally(h_->e, emitters.empty() ? nullptr : emitters.data(), &grid, tables.empty() ? nullptr : tables.data(),
                                                n_emit, surfels.data(), seeds, surfels.size(), &p, first_sample, samples,
                                                sums ? out.data() : nullptr, tally.empty() ? &none : tally.data()));
        return out;
    }
    void direct_light_grid_tally_device(const rb_emitter* d_emitters, const rb_probe_grid& grid, const uint32_t* d_tables, size_t n_emit,
                                        const rb_surfel* d_surfels, const uint32_t* d_seeds, size_t n, const rb_light_params& p,
                                        rb_radiance* d_out, rb_grid_tally* d_tally, uint32_t samples, uint32_t first_sample = 0) {
        check(h_->e, rb_direct_light_grid_tally_device(h_->e, d_emitters, &grid, d_tables, n_emit, d_surfels, d_seeds, n, &p, first_sample,
                                                       samples, d_out, d_tally));
    }
    static std::vector<uint32_t> emitter_grid_learned(const std::vector<rb_emitter>& emitters, const rb_probe_grid& grid,
                                                      const std::vector<rb_grid_tally>& tally, float prior = 1.0f, int32_t device = -1) {
        std::vector<uint32_t> out(emitters.size() * grid.counts[0] * grid.counts[1] * grid.counts[2]);
        if (tally.size() != out.size()) throw std::invalid_argument("emitter_grid_learned: one record per cell and emitter is needed");
        check(nullptr, rb_emitter_grid_learned(device, emitters.data(), emitters.size(), &grid, tally.data(), prior, out.data()));
        return out;
    }
    void emitter_grid_learned_device(const rb_emitter* d_emitters, size_t n_emit, const rb_probe_grid& grid, const rb_grid_tally* d_tally,
                                     float prior, uint32_t* d_tables_out) {
        check(h_->e, rb_emitter_grid_learned_device(h_->e, d_emitters, n_emit, &grid, d_tally, prior, d_tables_out));
    }
    // ---- lightmap texels made on the device (extension; rb_abi.h): the surfel of every texel of an atlas
    // over the scene's uvs, and the bake of the whole map in one call (rgba in sample_texture's layout, row 0 on top)
    static rb_lightmap_params lightmap_params(uint32_t width, uint32_t height, uint32_t mesh = RB_LIGHTMAP_ALL_MESHES, bool flip = false,
                                              float offset = 1e-3f, uint32_t dilate = 2) {
        rb_lightmap_params p{};
        p.width = width;
        p.height = height;
        p.mesh = mesh;
        p.flags = flip ? RB_LIGHTMAP_FLIP : 0u;
        p.offset = offset;
        p.dilate = dilate;
        return p;
    }
    std::vector<float> bake_lightmap(const rb_lightmap_params& p, uint32_t samples, uint32_t first_sample = 0, std::vector<rb_radiance>* sums = nullptr) {
        const size_t n = static_cast<size_t>(p.width) * p.height;
        std::vector<float> rgba(n * 4);
        if (sums) sums->resize(n);
        check(h_->e, rb_bake_lightmap(h_->e, &p, first_sample, samples, rgba.data(), sums ? sums->data() : nullptr));
        return rgba;
    }
    // the same on the engine's device memory: queued on the engine's stream -- sync() waits
    void lightmap_surfels_device(const rb_lightmap_params& p, rb_surfel* d_surfels, uint32_t* d_owners = nullptr) {
        check(h_->e, rb_lightmap_surfels_device(h_->e, &p, d_surfels, d_owners));
    }
    void bake_lightmap_device(const rb_lightmap_params& p, float* d_rgba, rb_radiance* d_sums, uint32_t samples, uint32_t first_sample = 0) {
        check(h_->e, rb_bake_lightmap_device(h_->e, &p, first_sample, samples, d_rgba, d_sums));
    }
    // ---- irradiance probes made on the device (extension; rb_abi.h): per probe the ordered SH9 sums over
    // `samples` uniform-sphere rays; the radiance coefficient j is (4 pi / weight) * sum[j]
    std::vector<rb_sh9> bake_probes(const std::vector<rb_probe>& probes, uint32_t samples, uint32_t first_sample = 0,
                                    const uint32_t* seeds = nullptr) {
        std::vector<rb_sh9> out(probes.size());
        check(h_->e, rb_bake_probes(h_->e, probes.data(), seeds, probes.size(), first_sample, samples, out.data()));
        return out;
    }
    // the same on the engine's device memory: queued on the engine's stream -- sync() waits
    void bake_probes_device(const rb_probe* d_probes, const uint32_t* d_seeds, size_t n, rb_sh9* d_out, uint32_t samples,
                            uint32_t first_sample = 0) {
        check(h_->e, rb_bake_probes_device(h_->e, d_probes, d_seeds, n, first_sample, samples, d_out));
    }
    // ---- light points from a baked probe grid (extension; rb_abi.h): the sums of bake_probes scaled to
    // irradiance-over-pi coefficients, and the blend of the eight probes of a regular grid round every point.  The host forms
    // need no engine: the work runs on `device` (-1: the current one).
    static std::vector<rb_sh9> probe_coefficients(const std::vector<rb_sh9>& sums, int32_t device = -1) {
        std::vector<rb_sh9> out(sums.size());
        check(nullptr, rb_probe_coefficients(device, sums.data(), sums.size(), out.data()));
        return out;
    }
    static std::vector<rb_lit> light_points(const rb_probe_grid& grid, const std::vector<rb_sh9>& coeffs, const std::vector<rb_surfel>& points,
                                            int32_t device = -1) {
        std::vector<rb_lit> out(points.size());
        check(nullptr, rb_light_points(device, &grid, coeffs.data(), points.data(), points.size(), out.data()));
        return out;
    }
    // the same on the engine's device memory (d_coeffs_out may be d_sums): queued on the engine's stream -- sync() waits
    void probe_coefficients_device(const rb_sh9* d_sums, size_t n, rb_sh9* d_coeffs_out) {
        check(h_->e, rb_probe_coefficients_device(h_->e, d_sums, n, d_coeffs_out));
    }
    void light_points_device(const rb_probe_grid& grid, const rb_sh9* d_coeffs, const rb_surfel* d_points, size_t m, rb_lit* d_out) {
        check(h_->e, rb_light_points_device(h_->e, &grid, d_coeffs, d_points, m, d_out));
    }
    // ---- probe visibility (extension; rb_abi.h): per probe an 8 x 8 octahedral map of the sums of the
    // first-hit distance, its square, the samples and the back faces among them; the moments of the sums with the share of
    // back faces per probe (above a quarter or so: the probe sits inside geometry); the blend with every corner weighed by
    // the map and by the wrapped cosine of the point's normal.  The forms without an engine run on `device` (-1: the current one).
    std::vector<rb_probe_depth> bake_probe_depth(const std::vector<rb_probe>& probes, uint32_t samples, float max_distance,
                                                 uint32_t first_sample = 0, const uint32_t* seeds = nullptr) {
        std::vector<rb_probe_depth> out(probes.size());
        check(h_->e, rb_bake_probe_depth(h_->e, probes.data(), seeds, probes.size(), first_sample, samples, max_distance, out.data()));
        return out;
    }
    void bake_probe_depth_device(const rb_probe* d_probes, const uint32_t* d_seeds, size_t n, rb_probe_depth* d_out, uint32_t samples,
                                 float max_distance, uint32_t first_sample = 0) {
        check(h_->e, rb_bake_probe_depth_device(h_->e, d_probes, d_seeds, n, first_sample, samples, max_distance, d_out));
    }
    static std::vector<rb_probe_depth> probe_moments(const std::vector<rb_probe_depth>& sums, std::vector<float>* backface_share = nullptr,
                                                     int32_t device = -1) {
        std::vector<rb_probe_depth> out(sums.size());
        if (backface_share) backface_share->assign(sums.size(), 0.0f);
        check(nullptr, rb_probe_moments(device, sums.data(), sums.size(), out.data(), backface_share ? backface_share->data() : nullptr));
        return out;
    }
    static std::vector<rb_lit> light_points_visible(const rb_probe_grid& grid, const std::vector<rb_sh9>& coeffs,
                                                    const std::vector<rb_probe_depth>& moments, const std::vector<rb_surfel>& points,
                                                    const rb_light_visibility& params, int32_t device = -1) {
        std::vector<rb_lit> out(points.size());
        check(nullptr, rb_light_points_visible(device, &grid, coeffs.data(), moments.empty() ? nullptr : moments.data(), points.data(),
                                               points.size(), &params, out.data()));
        return out;
    }
    // the same on the engine's device memory (d_moments_out may be d_sums, d_backface_share_out nullptr)
    void probe_moments_device(const rb_probe_depth* d_sums, size_t n, rb_probe_depth* d_moments_out, float* d_backface_share_out = nullptr) {
        check(h_->e, rb_probe_moments_device(h_->e, d_sums, n, d_moments_out, d_backface_share_out));
    }
    void light_points_visible_device(const rb_probe_grid& grid, const rb_sh9* d_coeffs, const rb_probe_depth* d_moments, const rb_surfel* d_points,
                                     size_t m, const rb_light_visibility& params, rb_lit* d_out) {
        check(h_->e, rb_light_points_visible_device(h_->e, &grid, d_coeffs, d_moments, d_points, m, &params, d_out));
    }
    void sync() { check(h_->e, rb_sync(h_->e)); }
    // ---- the denoiser (rb_abi.h): the a-trous filter over the committed accumulation
    static rb_denoise_params denoise_defaults() {
        rb_denoise_params p{};
        (void)rb_denoise_default_params(&p);
        return p;
    }
    // the RGBA8 frame (w * h * 4 bytes) and, if linear_out is not null, the linear vec4 output (w * h * 4 floats)
    std::vector<uint8_t> denoise(const rb_denoise_params& p = denoise_defaults(), std::vector<float>* linear_out = nullptr) {
        uint32_t w = 0, h = 0;
        check(h_->e, rb_get_size(h_->e, &w, &h));
        std::vector<uint8_t> rgba(static_cast<size_t>(w) * h * 4);
        if (linear_out) linear_out->resize(static_cast<size_t>(w) * h * 4);
        check(h_->e, rb_denoise(h_->e, &p, rgba.data(), linear_out ? linear_out->data() : nullptr));
        return rgba;
    }
    // outputs in the engine's device memory (either may be null, not both): queued, not waited for -- sync() waits
    void denoise_device(const rb_denoise_params& p, uint8_t* d_rgba_out, float* d_linear_out = nullptr) {
        check(h_->e, rb_denoise_device(h_->e, &p, d_rgba_out, d_linear_out));
    }
    std::vector<rb_guide> denoise_guides() {
        uint32_t w = 0, h = 0;
        check(h_->e, rb_get_size(h_->e, &w, &h));
        std::vector<rb_guide> g(static_cast<size_t>(w) * h);
        check(h_->e, rb_denoise_guides(h_->e, g.data()));
        return g;
    }
    // ---- temporal reprojection (rb_abi.h): the previous frame's history carried across a camera move
    static rb_view view_from_camera(const rb_camera& cam, uint32_t w, uint32_t h) {
        rb_view v{};
        check(nullptr, rb_view_from_camera(&cam, w, h, &v));
        return v;
    }
    static rb_reproject_params reproject_defaults() {
        rb_reproject_params p{};
        (void)rb_reproject_default_params(&p);
        return p;
    }
    // REPROJECT, with cur4 MERGE on top, on host arrays of w * h records; no engine
    static std::vector<float> reproject_buffers(const rb_reproject_params& p, uint32_t w, uint32_t h, const rb_view& prev_view,
                                                const std::vector<float>& prev4, const std::vector<rb_guide>& prev_guides,
                                                const std::vector<rb_guide>& cur_guides, const std::vector<float>* cur4 = nullptr, int32_t device = -1) {
        std::vector<float> out(static_cast<size_t>(w) * h * 4);
        check(nullptr, rb_reproject_buffers(device, &p, w, h, &prev_view, prev4.data(), prev_guides.data(), cur_guides.data(),
                                            cur4 ? cur4->data() : nullptr, out.data()));
        return out;
    }
    // the same on the engine's device memory (d_cur4 may be null): queued on the engine's stream -- sync() waits
    void reproject(const rb_reproject_params& p, uint32_t w, uint32_t h, const rb_view& prev_view, const float* d_prev4, const rb_guide* d_prev_guides,
                   const rb_guide* d_cur_guides, const float* d_cur4, float* d_out4) {
        check(h_->e, rb_reproject_device(h_->e, &p, w, h, &prev_view, d_prev4, d_prev_guides, d_cur_guides, d_cur4, d_out4));
    }
    // denoise() on the frame with its history; call once per displayed frame, after its passes
    std::vector<uint8_t> denoise_history(const rb_reproject_params& rp = reproject_defaults(), const rb_denoise_params& dp = denoise_defaults(),
                                         std::vector<float>* linear_out = nullptr) {
        uint32_t w = 0, h = 0;
        check(h_->e, rb_get_size(h_->e, &w, &h));
        std::vector<uint8_t> rgba(static_cast<size_t>(w) * h * 4);
        if (linear_out) linear_out->resize(static_cast<size_t>(w) * h * 4);
        check(h_->e, rb_denoise_history(h_->e, &rp, &dp, rgba.data(), linear_out ? linear_out->data() : nullptr));
        return rgba;
    }
    void denoise_history_device(const rb_reproject_params& rp, const rb_denoise_params& dp, uint8_t* d_rgba_out, float* d_linear_out = nullptr) {
        check(h_->e, rb_denoise_history_device(h_->e, &rp, &dp, d_rgba_out, d_linear_out));
    }
    // the frame records {mean r, g, b, count} of the most recent denoise_history, before the filter
    std::vector<float> history() {
        uint32_t w = 0, h = 0;
        check(h_->e, rb_get_size(h_->e, &w, &h));
        std::vector<float> f(static_cast<size_t>(w) * h * 4);
        check(h_->e, rb_history_read(h_->e, f.data()));
        return f;
    }
    void history_reset() { check(h_->e, rb_history_reset(h_->e)); }
    float last_reproject_ms() {
        float ms = 0.0f;
        check(h_->e, rb_last_reproject_ms(h_->e, &ms));
        return ms;
    }
    // the displayed pixel (px from the left, py from the top): "sphere 3" / "mesh 2, triangle 517" for a click
    rb_hit pick(uint32_t px, uint32_t py, rb_surface* surface = nullptr) {
        rb_hit hit{};
        check(h_->e, rb_pick(h_->e, px, py, &hit, surface));
        return hit;
    }
    rb_engine* raw() const { return h_->e; }
};

}  // namespace renderbaby
