// rb_camera.hip -- camera rays made on the device (rb_camera_rays, rb_trace_camera; DESIGN.md section 15, the normative
// definition): the ray of every (pixel, sample) item from the item's own random stream -- two jitter draws, then for a thin
// lens a rejection-sampled point on the lens disc --, for the perspective, orthographic and equirectangular cameras of
// rb_camera_ex.  One full-width pass, one lane per item, before the trace kernels (k_cam*, rb_radiance.hip) walk the records:
// done inside their refill it would run at the dozen lanes a refill serves (section 15.4: what that cost k_trace's much shorter
// path start).  Same numerics contract as rb_kernels.hip: every step one binary32 operation in the order written,
// no FMA contraction, correctly rounded / and sqrt, so that renderbaby_amd/camera.py equals this file bit for bit.
#include "rb_device_sincos.hpp"

#pragma clang fp contract(off)

namespace rb {
namespace {

// ========================================================= k_cam_rays ====
// lane = item.  Item order (the trace's scratch): item = (block * samples + sample) * 64 + pixel-in-block, block = 64
// consecutive pixels of the piece -- the order the k_cam kernels hand items out in, so a wave's 64 records are one contiguous
// 2 KiB.  Linear order (rb_camera_rays): item = (pixel - first_pixel) * samples + sample.
__global__ void __launch_bounds__(256) k_cam_rays(const CamGenArgs g) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const uint32_t S = g.samples;
    uint32_t pix, smp;
    if (g.linear != 0u) {
        if (t >= g.n) return;
        const uint32_t i = g.item_base + t;
        pix = i / S;
        smp = i - pix * S;
    } else {
        const uint32_t row = t >> 6, blk = row / S;
        smp = row - blk * S;
        pix = blk * 64u + (t & 63u);
        if (pix >= g.n) return;   // the padding of the last block, and the lanes behind the last row
    }
    const rb_camera_ex& c = g.cam;
    const uint32_t p = g.first_pixel + pix;
    const uint32_t prow = p / c.width, pcol = p - prow * c.width;
    const f3 pos = mk(c.pos[0], c.pos[1], c.pos[2]), right = mk(c.right[0], c.right[1], c.right[2]),
             up = mk(c.up[0], c.up[1], c.up[2]), fwd = mk(c.forward[0], c.forward[1], c.forward[2]);

    uint32_t seed = pcg(p + pcg(g.first_sample + smp));
    float jx = rnd(seed) - 0.5f, jy = rnd(seed) - 0.5f;
    if ((c.flags & RB_CAM_NO_JITTER) != 0u) jx = jy = 0.0f;
    const float sx = ((((float)pcol + 0.5f) + jx) / (float)c.width) * 2.0f - 1.0f;
    const float sy = 1.0f - ((((float)prow + 0.5f) + jy) / (float)c.height) * 2.0f;

    f3 o = pos, d;
    if (c.kind == RB_CAM_PERSPECTIVE) {
        const float a = c.tan_half_fov * ((float)c.width / (float)c.height);
        d = ((sx * a) * right + (sy * c.tan_half_fov) * up) + fwd;
        if (c.lens_radius != 0.0f) {
            float lx, ly;
            for (;;) {
                lx = rnd_pm1(seed);
                ly = rnd_pm1(seed);
                if (lx * lx + ly * ly < 1.0f) break;
            }
            o = (pos + (c.lens_radius * lx) * right) + (c.lens_radius * ly) * up;
            d = (pos + c.focus_distance * d) - o;
        }
    } else if (c.kind == RB_CAM_ORTHO) {
        o = (pos + (sx * c.half_width) * right) + (sy * c.half_height) * up;
        d = fwd;
    } else {
        const SinCos lon = sincos_turn(sx), lat = sincos_turn(0.5f * sy);
        d = ((lat.c * lon.s) * right + lat.s * up) + (lat.c * lon.c) * fwd;
    }
    d = normalize(d);
    // rb_cast_rays' rule; an invalid ray is marked by a zero direction
    if (!(finite3(o) && finite3(d)) || zero3(d)) d = mk(0, 0, 0);

    store_record(g.recs, g.seeds, t, o, d, seed);
}

}  // namespace

// One piece: every record of it, queued on `stream`; nothing is waited for.  Item order: g.n pixels, rounded up to whole
// blocks of 64 (the records of the padding are not written, the trace kernels do not read them); linear order: g.n items.
int launch_camera_rays(const CamGenArgs& g, void* stream_) {
    if (g.n == 0u) return 0;
    if (g.recs == nullptr || g.samples == 0u || g.cam.width == 0u || g.cam.height == 0u) return (int)hipErrorInvalidValue;
    if (g.linear == 0u && g.seeds != nullptr) return (int)hipErrorInvalidValue;
    const uint64_t lanes = g.linear != 0u ? (uint64_t)g.n : (((uint64_t)g.n + 63u) / 64u) * 64u * g.samples;
    if (lanes > 0x7FFFFFFFull) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_cam_rays, dim3((uint32_t)((lanes + 255u) / 256u)), dim3(256), 0, static_cast<hipStream_t>(stream_), g);
    return (int)hipGetLastError();
}

}  // namespace rb
