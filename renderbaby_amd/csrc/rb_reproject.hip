// rb_reproject.hip -- temporal reprojection: the previous frame's history carried across a camera move (rb_reproject*,
// rb_denoise_history; DESIGN.md section 22, the normative definition; renderbaby_amd/temporal.py restates it in numpy).  Same
// numerics contract as rb_denoise.hip (no FMA contraction, correctly rounded /): every arithmetic step below is ONE binary32
// operation, in the order section 22.1 fixes, so the device's records equal the host model's bit for bit.  "max(a, b)" is
// `a > b ? a : b`, "min(a, b)" `a < b ? a : b`, never fmaxf / fminf.
//   k_reproject<HAS_CUR>   REPROJECT of one pixel, with HAS_CUR MERGE onto cur4 fused behind it
//   k_history_merge        MERGE of a base plane and the accumulation (mirrored here, sum / w as k_dn_prepare has it)
// The guide planes and their layout are rb_denoise.hip's (launch_guide_split makes them from rb_guide records).
// A wave of k_reproject is 64 consecutive pixels of one row: its three current guide quads, its cur4 and its output are one
// contiguous KiB each.  The four previous taps are gathers of 16-byte quads from four planes; under a small camera motion
// neighbouring lanes land on neighbouring texels, so a wave's gathers are a few cache lines per plane and row.
#include "rb_device_common.hpp"

#include <cmath>

#pragma clang fp contract(off)

namespace rb {
namespace {

constexpr uint32_t kRpBlock = 256;
typedef const v4f* __restrict__ q4p;

DEV uint32_t fbits(float f) { return __float_as_uint(f); }
DEV bool finite1(float f) { return (fbits(f) & 0x7F800000u) != 0x7F800000u; }
DEV bool finite4(v4f v) { return finite1(v.x) && finite1(v.y) && finite1(v.z) && finite1(v.w); }
DEV float max_gt(float a, float b) { return a > b ? a : b; }
DEV float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

struct RpArgs {
    uint32_t w, h, tiles_x;
    rb_view v;
    float sigma_depth, normal_min, albedo_floor, max_history;
    q4p prev4, pnt, ppc, pal;   // the previous frame: colour | count, normal | t, position | class, albedo
    q4p cnt, cpc, cal;          // the current guides
    q4p cur4;                   // HAS_CUR
    v4f* out;
};

// MERGE of section 22.1: hst onto cur = {c, n} of a pixel of class cls
DEV v4f merge1(uint32_t cls, v4f hst, v4f cur) {
    if (cls == 0u || !finite4(cur) || !(cur.w >= 0.0f) || hst.w == 0.0f) return cur;
    const float tot = hst.w + cur.w;
    v4f o;
    o.x = (hst.x * hst.w + cur.x * cur.w) / tot;
    o.y = (hst.y * hst.w + cur.y * cur.w) / tot;
    o.z = (hst.z * hst.w + cur.z * cur.w) / tot;
    o.w = tot;
    return o;
}

// Block = 64 x 4 pixels, a wave one row of it (as k_dn_iter).
template <bool HAS_CUR>
__global__ void __launch_bounds__(kRpBlock) k_reproject(const RpArgs a) {
    const uint32_t bx = blockIdx.x % a.tiles_x, by = blockIdx.x / a.tiles_x;
    const int x = (int)(bx * 64u + (threadIdx.x & 63u)), y = (int)(by * 4u + (threadIdx.x >> 6));
    const int w = (int)a.w, h = (int)a.h;
    if (x >= w || y >= h) return;
    const size_t i = (size_t)y * a.w + (uint32_t)x;
    const v4f gp = a.cpc[i], gn = a.cnt[i], ga = a.cal[i];
    v4f cur = {0.0f, 0.0f, 0.0f, 0.0f};
    if (HAS_CUR) cur = a.cur4[i];
    const uint32_t cls = fbits(gp.w);
    // where the pixel's first hit was on screen under the previous camera
    const float ex = gp.x - a.v.pos[0], ey = gp.y - a.v.pos[1], ez = gp.z - a.v.pos[2];
    const float z = dot3(ex, ey, ez, a.v.fwd[0], a.v.fwd[1], a.v.fwd[2]);
    const float pa = dot3(ex, ey, ez, a.v.right[0], a.v.right[1], a.v.right[2]);
    const float pb = dot3(ex, ey, ez, a.v.up[0], a.v.up[1], a.v.up[2]);
    const float X = a.v.cx - (pa / z) * a.v.sx;
    const float Y = a.v.cy - (pb / z) * a.v.sy;
    const bool on = cls != 0u && z > 0.0f && X > -1.0f && X < (float)w && Y > -1.0f && Y < (float)h;
    // (no float becomes an integer before the test has passed: a pixel without history taps texel 0 and masks it)
    const float Xs = on ? X : 0.0f, Ys = on ? Y : 0.0f;
    const float X0 = __builtin_floorf(Xs), Y0 = __builtin_floorf(Ys);
    const float fx = Xs - X0, fy = Ys - Y0;
    const int ix = (int)X0, iy = (int)Y0;
    const float wx[2] = {1.0f - fx, fx}, wy[2] = {1.0f - fy, fy};
    // the four taps: all loads first, from addresses clamped into the frame, then the tests and the sums of those that count
    v4f c4[4], nq[4], pq[4], aq[4];
    bool in[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const int qx = ix + (t & 1), qy = iy + (t >> 1);
        in[t] = on && qx >= 0 && qx < w && qy >= 0 && qy < h;
        const size_t q = (size_t)(qy < 0 ? 0 : qy >= h ? h - 1 : qy) * a.w + (uint32_t)(qx < 0 ? 0 : qx >= w ? w - 1 : qx);
        c4[t] = a.prev4[q];
        nq[t] = a.pnt[q];
        pq[t] = a.ppc[q];
        aq[t] = a.pal[q];
    }
    const float mx = max_gt(ga.x, a.albedo_floor), my = max_gt(ga.y, a.albedo_floor), mz = max_gt(ga.z, a.albedo_floor);
    const float den = a.sigma_depth * gn.w;
    float hx = 0.0f, hy = 0.0f, hz = 0.0f, hn = 0.0f, bs = 0.0f;
#pragma unroll
    for (int t = 0; t < 4; t++) {   // dy = 0, 1 outside, dx = 0, 1 inside
        const float bw = wx[t & 1] * wy[t >> 1];
        const float dn = dot3(gn.x, gn.y, gn.z, nq[t].x, nq[t].y, nq[t].z);
        const float dist = __builtin_fabsf(dot3(gn.x, gn.y, gn.z, pq[t].x - gp.x, pq[t].y - gp.y, pq[t].z - gp.z));
        const bool take = in[t] && bw > 0.0f && fbits(pq[t].w) == cls && finite4(c4[t]) && c4[t].w > 0.0f && dn >= a.normal_min && dist <= den;
        if (take) {
            hx = hx + bw * (c4[t].x / max_gt(aq[t].x, a.albedo_floor));
            hy = hy + bw * (c4[t].y / max_gt(aq[t].y, a.albedo_floor));
            hz = hz + bw * (c4[t].z / max_gt(aq[t].z, a.albedo_floor));
            hn = hn + bw * c4[t].w;
            bs = bs + bw;
        }
    }
    v4f hst = {0.0f, 0.0f, 0.0f, 0.0f};
    if (bs > 0.0f) {
        v4f r;
        r.x = (hx / bs) * mx;
        r.y = (hy / bs) * my;
        r.z = (hz / bs) * mz;
        const float hl = hn / bs;
        r.w = hl < a.max_history ? hl : a.max_history;
        if (finite4(r)) hst = r;
    }
    a.out[i] = HAS_CUR ? merge1(cls, hst, cur) : hst;
}

// F = MERGE(base, {mean radiance, acc.w}): the accumulation is in shader x order, everything else in the frame's
__global__ void __launch_bounds__(kRpBlock) k_history_merge(uint32_t w, uint32_t n, q4p accum, q4p base, q4p pc, v4f* __restrict__ out) {
    const uint32_t i = blockIdx.x * kRpBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t y = i / w, xd = i - y * w;
    const v4f acc = accum[(size_t)y * w + (w - 1u - xd)];
    v4f cur = {0.0f, 0.0f, 0.0f, acc.w};
    if (!(acc.w == 0.0f)) {
        cur.x = acc.x / acc.w;   // as k_dn_prepare (section 13.1)
        cur.y = acc.y / acc.w;
        cur.z = acc.z / acc.w;
    }
    out[i] = merge1(fbits(pc[i].w), base[i], cur);
}

}  // namespace

bool reproject_params_valid(const rb_reproject_params& p, const char** why) {
    const char* w = nullptr;
    if (!std::isfinite(p.sigma_depth) || !(p.sigma_depth > 0.0f)) w = "sigma_depth is not a finite positive number";
    else if (!std::isfinite(p.normal_min) || !(p.normal_min >= -1.0f && p.normal_min <= 1.0f)) w = "normal_min is not within -1 .. 1";
    else if (!std::isfinite(p.albedo_floor) || !(p.albedo_floor > 0.0f)) w = "albedo_floor is not a finite positive number";
    else if (!std::isfinite(p.max_history) || !(p.max_history >= 1.0f)) w = "max_history is not a finite number of at least 1";
    else if (p.flags != 0u || p._reserved[0] != 0u || p._reserved[1] != 0u || p._reserved[2] != 0u) w = "flags and the reserved words must be 0";
    if (why) *why = w;
    return w == nullptr;
}

bool view_finite(const rb_view& v) {
    const float* f = v.pos;   // sixteen floats, no padding (rb_abi.h asserts the size)
    for (int k = 0; k < 16; k++)
        if (!std::isfinite(f[k])) return false;
    return true;
}

int launch_reproject(const rb_reproject_params& prm, const ReprojectArgs& r, void* stream) {
    const size_t n = (size_t)r.w * r.h;
    if (n == 0u) return 0;
    if (n >= (1ull << 31)) return (int)hipErrorInvalidValue;
    RpArgs a{};
    a.w = r.w;
    a.h = r.h;
    a.tiles_x = (r.w + 63u) / 64u;
    a.v = r.view;
    a.sigma_depth = prm.sigma_depth;
    a.normal_min = prm.normal_min;
    a.albedo_floor = prm.albedo_floor;
    a.max_history = prm.max_history;
    a.prev4 = (q4p)r.prev4;
    a.pnt = (q4p)r.prev.nt;
    a.ppc = (q4p)r.prev.pc;
    a.pal = (q4p)r.prev.al;
    a.cnt = (q4p)r.cur.nt;
    a.cpc = (q4p)r.cur.pc;
    a.cal = (q4p)r.cur.al;
    a.cur4 = (q4p)r.cur4;
    a.out = (v4f*)r.out4;
    const dim3 grid(a.tiles_x * ((r.h + 3u) / 4u)), block(kRpBlock);
    if (r.cur4) hipLaunchKernelGGL(k_reproject<true>, grid, block, 0, static_cast<hipStream_t>(stream), a);
    else hipLaunchKernelGGL(k_reproject<false>, grid, block, 0, static_cast<hipStream_t>(stream), a);
    return (int)hipGetLastError();
}

int launch_history_merge(uint32_t w, uint32_t h, const float* accum, const float* base, const GuidePlanes& g, float* out4, void* stream) {
    const size_t n = (size_t)w * h;
    if (n == 0u) return 0;
    if (n >= (1ull << 31)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_history_merge, dim3((uint32_t)((n + kRpBlock - 1u) / kRpBlock)), dim3(kRpBlock), 0, static_cast<hipStream_t>(stream), w,
                       (uint32_t)n, (q4p)accum, (q4p)base, (q4p)g.pc, (v4f*)out4);
    return (int)hipGetLastError();
}

}  // namespace rb
