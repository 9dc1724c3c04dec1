// rb_denoise.hip -- the edge-avoiding a-trous wavelet filter over the first-hit buffers (rb_denoise*; DESIGN.md section 13,
// the normative definition; renderbaby_amd/denoise.py restates it in numpy).  Same numerics contract as the other device files
// (no FMA contraction, correctly rounded / and sqrt): every arithmetic step below is ONE binary32 operation, in the order
// section 13 fixes, so the device's frames equal the host model's bit for bit.  "max(a, b)" is `a > b ? a : b` throughout
// (a NaN first operand yields b), never fmaxf.
//   k_guide_pack      first-hit records of the pixel centres -> the guide planes (once per accepted update)
//   k_guide_split     rb_guide records -> planes (rb_denoise_buffers), k_guide_join: planes -> records (rb_denoise_guides)
//   k_dn_prepare      accumulation (mirrored here) or mean radiance -> demodulated colour | class
//   k_dn_iter         one iteration, 25 taps at distance `step`; every tap three 16-byte loads through L1 / L2
//   k_dn_iter_lds     the same for steps 1 and 2 from a 16 x 16 tile staged in LDS with its halo
//   k_dn_finish       remodulate, linear vec4 and / or tone map + RGBA8
// The work is memory- and L2-bound: per pixel and iteration up to 25 x 48 bytes of taps against ~40 VALU operations and three
// divisions per tap.  A wave of k_dn_iter is 64 consecutive pixels of one row, so every tap load of a wave is one contiguous
// KiB, the five taps of a row overlap in L1, and the row predicates are wave-uniform.
#include "rb_device_centre.hpp"

#include <cmath>
#include <cstdlib>

#pragma clang fp contract(off)

namespace rb {
namespace {

constexpr uint32_t kDnBlock = 256;
// steps 1 and 2 from LDS: 0.214 against 0.258 ms for the two iterations at 1920 x 1080 on C2, 0.133 against 0.144 ms on C3, 0.038 / 0.043
// and 0.032 / 0.036 ms at 512 x 512 (profiles/r09_denoise_rate.txt)
constexpr uint32_t kDenoiseDefaultVariant = kDenoiseLds;
typedef const v4f* __restrict__ q4p;

DEV uint32_t fbits(float f) { return __float_as_uint(f); }
DEV bool finite1(float f) { return (fbits(f) & 0x7F800000u) != 0x7F800000u; }
DEV float max_gt(float a, float b) { return a > b ? a : b; }

// what an iteration needs beside its buffers
struct DnIter {
    uint32_t w, h, tiles_x;
    int step;
    uint32_t npow;       // normal_power_log2
    float sigma_depth;
    float sigma2;        // sigma_i * sigma_i, sigma_i = sigma_color * 2^-i (worked out on the host: two binary32 multiplications)
    uint32_t use_color;  // sigma_color > 0
};

struct DnSum {
    float x, y, z, w;
};

// h[|d|] * h[|e|], h = (3/8, 1/4, 1/16): every product is exact in binary32
DEV float tap_kernel(int dx, int dy) {
    const float hx = dx == 0 ? 0.375f : (dx == 1 || dx == -1) ? 0.25f : 0.0625f;
    const float hy = dy == 0 ? 0.375f : (dy == 1 || dy == -1) ? 0.25f : 0.0625f;
    return hx * hy;
}

// one accepted tap (section 13, "Iteration"): rp / np / pp the centre's colour | class, normal | t, position; *q the tap's
DEV void tap_add(const DnIter& c, float k, v4f rp, v4f np, v4f pp, float den, v4f rq, v4f nq, v4f pq, DnSum& s) {
    float wn = max_gt((np.x * nq.x + np.y * nq.y) + np.z * nq.z, 0.0f);
    for (uint32_t j = 0; j < c.npow; j++) wn = wn * wn;
    const float ex = pq.x - pp.x, ey = pq.y - pp.y, ez = pq.z - pp.z;
    const float dist = __builtin_fabsf((np.x * ex + np.y * ey) + np.z * ez);
    const float wz = max_gt(1.0f - dist / den, 0.0f);
    float w = (k * wn) * wz;
    if (c.use_color) {
        const float cx = rq.x - rp.x, cy = rq.y - rp.y, cz = rq.z - rp.z;
        const float d2 = (cx * cx + cy * cy) + cz * cz;
        const float wc = 1.0f / (1.0f + d2 / c.sigma2);
        w = w * wc;
    }
    s.x = s.x + w * rq.x;
    s.y = s.y + w * rq.y;
    s.z = s.z + w * rq.z;
    s.w = s.w + w;
}

DEV v4f tap_result(v4f rp, const DnSum& s) {
    v4f out = rp;   // the class travels on in .w
    if (s.w != 0.0f) {
        out.x = s.x / s.w;
        out.y = s.y / s.w;
        out.z = s.z / s.w;
    }
    return out;
}

// ---- one iteration, taps from global memory.  Block = 64 x 4 pixels, a wave one row of it.
__global__ void __launch_bounds__(kDnBlock) k_dn_iter(const DnIter c, q4p rin, q4p nt, q4p pc, v4f* __restrict__ rout) {
    const uint32_t bx = blockIdx.x % c.tiles_x, by = blockIdx.x / c.tiles_x;
    const int x = (int)(bx * 64u + (threadIdx.x & 63u)), y = (int)(by * 4u + (threadIdx.x >> 6));
    const int w = (int)c.w, h = (int)c.h;
    if (x >= w || y >= h) return;
    const size_t i = (size_t)y * c.w + (uint32_t)x;
    const v4f rp = rin[i];
    const uint32_t cls = fbits(rp.w);
    if (cls == 0u) {   // pass-through: copied, gives nothing, takes nothing
        rout[i] = rp;
        return;
    }
    const v4f np = nt[i], pp = pc[i];
    const float den = c.sigma_depth * np.w;
    DnSum s{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + dy * c.step;
        if (qy < 0 || qy >= h) continue;   // (the same for the whole wave)
        const size_t row = (size_t)qy * c.w;
        // the row's five taps: all loads first, from addresses clamped into the row, then the arithmetic of those that count
        v4f rq[5], nq[5], pq[5];
#pragma unroll
        for (int k = 0; k < 5; k++) {
            const int qx = x + (k - 2) * c.step;
            const size_t q = row + (uint32_t)(qx < 0 ? 0 : qx >= w ? w - 1 : qx);
            rq[k] = rin[q];
            nq[k] = nt[q];
            pq[k] = pc[q];
        }
#pragma unroll
        for (int k = 0; k < 5; k++) {
            const int qx = x + (k - 2) * c.step;
            if (qx >= 0 && qx < w && fbits(rq[k].w) == cls) tap_add(c, tap_kernel(k - 2, dy), rp, np, pp, den, rq[k], nq[k], pq[k], s);
        }
    }
    rout[i] = tap_result(rp, s);
}

// ---- the same for STEP 1 and 2 from LDS: a 16 x 16 tile with its halo of 2 * STEP pixels, three planes of quads
// (20 x 20 x 48 B = 18.75 KiB, 24 x 24 x 48 B = 27 KiB).  A staged pixel outside the frame gets class 0, which no filtered
// pixel has, so the class test skips it as the frame test of k_dn_iter does: the same taps in the same order.
template <int STEP>
__global__ void __launch_bounds__(kDnBlock) k_dn_iter_lds(const DnIter c, q4p rin, q4p nt, q4p pc, v4f* __restrict__ rout) {
    constexpr int H = 2 * STEP, S = 16 + 2 * H;
    __shared__ v4f s_r[S * S], s_n[S * S], s_p[S * S];
    const uint32_t bx = blockIdx.x % c.tiles_x, by = blockIdx.x / c.tiles_x;
    const int w = (int)c.w, h = (int)c.h;
    const int x0 = (int)(bx * 16u) - H, y0 = (int)(by * 16u) - H;
    for (int j = (int)threadIdx.x; j < S * S; j += (int)kDnBlock) {
        const int ly = j / S, lx = j - ly * S, gx = x0 + lx, gy = y0 + ly;
        v4f r = {0.0f, 0.0f, 0.0f, 0.0f}, n = r, p = r;
        if (gx >= 0 && gy >= 0 && gx < w && gy < h) {
            const size_t q = (size_t)gy * c.w + (uint32_t)gx;
            r = rin[q];
            n = nt[q];
            p = pc[q];
        }
        s_r[j] = r;
        s_n[j] = n;
        s_p[j] = p;
    }
    __syncthreads();
    const int tx = (int)(threadIdx.x & 15u), ty = (int)(threadIdx.x >> 4);
    const int x = (int)(bx * 16u) + tx, y = (int)(by * 16u) + ty;
    if (x >= w || y >= h) return;
    const size_t i = (size_t)y * c.w + (uint32_t)x;
    const int lc = (ty + H) * S + tx + H;
    const v4f rp = s_r[lc];
    const uint32_t cls = fbits(rp.w);
    if (cls == 0u) {
        rout[i] = rp;
        return;
    }
    const v4f np = s_n[lc], pp = s_p[lc];
    const float den = c.sigma_depth * np.w;
    DnSum s{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int lq = lc + dy * STEP * S + dx * STEP;   // inside the staged square by construction
            const v4f rq = s_r[lq];
            if (fbits(rq.w) == cls) tap_add(c, tap_kernel(dx, dy), rp, np, pp, den, rq, s_n[lq], s_p[lq], s);
        }
    }
    rout[i] = tap_result(rp, s);
}

// ---- prepare: mean radiance (mirrored out of the accumulation), the non-finite rule, demodulation
struct DnPrep {
    uint32_t w, n;
    q4p accum, color4, pc, al;
    float floor;
    uint32_t demod;   // iterations > 0
    v4f* r0;
};
__global__ void __launch_bounds__(kDnBlock) k_dn_prepare(const DnPrep a) {
    const uint32_t i = blockIdx.x * kDnBlock + threadIdx.x;
    if (i >= a.n) return;
    v4f c;
    if (a.accum != nullptr) {
        const uint32_t y = i / a.w, xd = i - y * a.w;
        const v4f acc = a.accum[(size_t)y * a.w + (a.w - 1u - xd)];
        if (acc.w == 0.0f) {
            c = v4f{0.0f, 0.0f, 0.0f, 0.0f};
        } else {
            c.x = acc.x / acc.w;   // shader.wgsl:720
            c.y = acc.y / acc.w;
            c.z = acc.z / acc.w;
        }
    } else {
        c = a.color4[i];
    }
    uint32_t cls = fbits(a.pc[i].w);
    if (!(finite1(c.x) && finite1(c.y) && finite1(c.z))) cls = 0u;
    if (a.demod && cls != 0u) {
        const v4f al = a.al[i];
        c.x = c.x / max_gt(al.x, a.floor);
        c.y = c.y / max_gt(al.y, a.floor);
        c.z = c.z / max_gt(al.z, a.floor);
    }
    c.w = __uint_as_float(cls);
    a.r0[i] = c;
}

// ---- finish: remodulate, the linear vec4, shader.wgsl:721-722 + color_map (:137-151, with its clamp to [0, 1])
struct DnFinish {
    uint32_t n;
    q4p r, al;
    float floor;
    uint32_t remod;
    v4f* linear;
    uint32_t* rgba;
};
DEV uint32_t map8(float o) {
    const float m = o / (o + 1.0f);
    float g = (m > 0.0f) ? sqrtf(m) : 0.0f;
    g = g > 1.0f ? 1.0f : g;
    return f2u(g * 255.999f);
}
__global__ void __launch_bounds__(kDnBlock) k_dn_finish(const DnFinish a) {
    const uint32_t i = blockIdx.x * kDnBlock + threadIdx.x;
    if (i >= a.n) return;
    const v4f r = a.r[i];
    v4f o = r;
    if (a.remod && fbits(r.w) != 0u) {
        const v4f al = a.al[i];
        o.x = r.x * max_gt(al.x, a.floor);
        o.y = r.y * max_gt(al.y, a.floor);
        o.z = r.z * max_gt(al.z, a.floor);
    }
    o.w = 1.0f;
    if (a.linear != nullptr) a.linear[i] = o;
    if (a.rgba != nullptr) a.rgba[i] = (255u << 24) | (map8(o.z) << 16) | (map8(o.y) << 8) | map8(o.x);
}

// ---- the guide planes
__global__ void __launch_bounds__(kDnBlock) k_guide_pack(const Cam cam, uint32_t w, uint32_t n, q4p hits, q4p surf, const GuidePlanes g) {
    const uint32_t i = blockIdx.x * kDnBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t y = i / w, xd = i - y * w;
    const v4f h0 = hits[(size_t)i * 3u], h2 = hits[(size_t)i * 3u + 2u];   // t kind prim mesh | normal -
    const v4f s0 = surf[(size_t)i * 3u], s1 = surf[(size_t)i * 3u + 1u];   // albedo flags | emissive texture
    const f3 d = centre_ray_dir(cam, w - 1u - xd, y);   // the query kernel's direction for this pixel, bit for bit
    const f3 pos = ld3(cam.pos) + h0.x * d;
    const uint32_t kind = fbits(h0.y);
    const bool surface = kind == RB_HIT_GROUND || kind == RB_HIT_TRIANGLE || kind == RB_HIT_SPHERE;
    const bool emits = s1.x > 0.0f || s1.y > 0.0f || s1.z > 0.0f;
    const uint32_t cls = (surface && !emits) ? kind : 0u;
    ((v4f*)g.nt)[i] = v4f{h2.x, h2.y, h2.z, h0.x};
    ((v4f*)g.pc)[i] = v4f{pos.x, pos.y, pos.z, __uint_as_float(cls)};
    ((v4f*)g.al)[i] = v4f{s0.x, s0.y, s0.z, 0.0f};
}
__global__ void __launch_bounds__(kDnBlock) k_guide_split(q4p guides, uint32_t n, const GuidePlanes g) {
    const uint32_t i = blockIdx.x * kDnBlock + threadIdx.x;
    if (i >= n) return;
    ((v4f*)g.nt)[i] = guides[(size_t)i * 3u];
    ((v4f*)g.pc)[i] = guides[(size_t)i * 3u + 1u];
    ((v4f*)g.al)[i] = guides[(size_t)i * 3u + 2u];
}
__global__ void __launch_bounds__(kDnBlock) k_guide_join(const GuidePlanes g, uint32_t n, v4f* __restrict__ guides) {
    const uint32_t i = blockIdx.x * kDnBlock + threadIdx.x;
    if (i >= n) return;
    guides[(size_t)i * 3u] = ((const v4f*)g.nt)[i];
    guides[(size_t)i * 3u + 1u] = ((const v4f*)g.pc)[i];
    guides[(size_t)i * 3u + 2u] = ((const v4f*)g.al)[i];
}

uint32_t blocks_for(size_t n) { return (uint32_t)((n + kDnBlock - 1u) / kDnBlock); }

}  // namespace

bool denoise_params_valid(const rb_denoise_params& p, const char** why) {
    const char* w = nullptr;
    if (p.iterations > 8u) w = "iterations is above 8";
    else if (p.normal_power_log2 > 10u) w = "normal_power_log2 is above 10";
    else if (!std::isfinite(p.sigma_depth) || !(p.sigma_depth > 0.0f)) w = "sigma_depth is not a finite positive number";
    else if (!std::isfinite(p.sigma_color)) w = "sigma_color is not finite";
    else if (!std::isfinite(p.albedo_floor) || !(p.albedo_floor > 0.0f)) w = "albedo_floor is not a finite positive number";
    else if (p.flags != 0u || p._reserved[0] != 0u || p._reserved[1] != 0u) w = "flags and the reserved words must be 0";
    if (why) *why = w;
    return w == nullptr;
}

int launch_denoise(const rb_denoise_params& prm, const DenoiseArgs& a, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const size_t n = (size_t)a.w * a.h;
    if (n == 0u) return 0;
    if (n >= (1ull << 31) || (a.linear_out == nullptr && a.rgba_out == nullptr)) return (int)hipErrorInvalidValue;
    uint32_t variant = a.variant;
    if (variant == 0u) {
        const char* env = std::getenv("RB_DENOISE_VARIANT");   // measurements: "plain" | "lds"
        variant = env && env[0] == 'l' ? kDenoiseLds : env && env[0] == 'p' ? kDenoisePlain : kDenoiseDefaultVariant;
    }
    const dim3 block(kDnBlock);
    DnPrep pr{};
    pr.w = a.w;
    pr.n = (uint32_t)n;
    pr.accum = (q4p)a.accum;
    pr.color4 = (q4p)a.color4;
    pr.pc = (q4p)a.g.pc;
    pr.al = (q4p)a.g.al;
    pr.floor = prm.albedo_floor;
    pr.demod = prm.iterations > 0u ? 1u : 0u;
    pr.r0 = (v4f*)a.r[0];
    hipLaunchKernelGGL(k_dn_prepare, dim3(blocks_for(n)), block, 0, stream, pr);
    int cur = 0;
    for (uint32_t i = 0; i < prm.iterations; i++) {
        DnIter c{};
        c.w = a.w;
        c.h = a.h;
        c.step = 1 << i;
        c.npow = prm.normal_power_log2;
        c.sigma_depth = prm.sigma_depth;
        const float sigma_i = prm.sigma_color * std::ldexp(1.0f, -(int)i);
        c.sigma2 = sigma_i * sigma_i;
        c.use_color = prm.sigma_color > 0.0f ? 1u : 0u;
        q4p rin = (q4p)a.r[cur];
        v4f* rout = (v4f*)a.r[1 - cur];
        if (variant == kDenoiseLds && c.step <= 2) {
            c.tiles_x = (a.w + 15u) / 16u;
            const dim3 grid(c.tiles_x * ((a.h + 15u) / 16u));
            if (c.step == 1) hipLaunchKernelGGL(k_dn_iter_lds<1>, grid, block, 0, stream, c, rin, (q4p)a.g.nt, (q4p)a.g.pc, rout);
            else hipLaunchKernelGGL(k_dn_iter_lds<2>, grid, block, 0, stream, c, rin, (q4p)a.g.nt, (q4p)a.g.pc, rout);
        } else {
            c.tiles_x = (a.w + 63u) / 64u;
            const dim3 grid(c.tiles_x * ((a.h + 3u) / 4u));
            hipLaunchKernelGGL(k_dn_iter, grid, block, 0, stream, c, rin, (q4p)a.g.nt, (q4p)a.g.pc, rout);
        }
        cur = 1 - cur;
    }
    DnFinish f{};
    f.n = (uint32_t)n;
    f.r = (q4p)a.r[cur];
    f.al = (q4p)a.g.al;
    f.floor = prm.albedo_floor;
    f.remod = pr.demod;
    f.linear = (v4f*)a.linear_out;
    f.rgba = a.rgba_out;
    hipLaunchKernelGGL(k_dn_finish, dim3(blocks_for(n)), block, 0, stream, f);
    return (int)hipGetLastError();
}

int launch_guide_pack(const rb_uniforms& u, const rb_hit* hits, const rb_surface* surf, uint32_t w, uint32_t h, const GuidePlanes& g, void* stream) {
    const size_t n = (size_t)w * h;
    if (n == 0u) return 0;
    if (n >= (1ull << 31)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_guide_pack, dim3(blocks_for(n)), dim3(kDnBlock), 0, static_cast<hipStream_t>(stream), host_cam(u), w, (uint32_t)n, (q4p)hits,
                       (q4p)surf, g);
    return (int)hipGetLastError();
}

int launch_guide_split(const rb_guide* guides, size_t n, const GuidePlanes& g, void* stream) {
    if (n == 0u) return 0;
    if (n >= (1ull << 31)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_guide_split, dim3(blocks_for(n)), dim3(kDnBlock), 0, static_cast<hipStream_t>(stream), (q4p)guides, (uint32_t)n, g);
    return (int)hipGetLastError();
}

int launch_guide_join(const GuidePlanes& g, size_t n, rb_guide* guides, void* stream) {
    if (n == 0u) return 0;
    if (n >= (1ull << 31)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_guide_join, dim3(blocks_for(n)), dim3(kDnBlock), 0, static_cast<hipStream_t>(stream), g, (uint32_t)n, (v4f*)guides);
    return (int)hipGetLastError();
}

}  // namespace rb
