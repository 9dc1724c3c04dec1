// rb_tri_filter.hpp -- the triangle sift of the single-node kernels ("The triangle sift"): the group records
// pass 1 tests, the origin region with its scene-wide Sp, and the decision whether a launch sifts at all.  Host code only, no HIP,
// double arithmetic with every stored value rounded to the safe side (rb_chunk_math.hpp's habits), so that a stand-alone program
// can exercise it (tests/test_tri_filter_plan.py).  The kernel side is sift_triangles in rb_device_intersect.hpp;
// renderbaby_amd/tri_filter_model.py restates both in numpy.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "rb_chunk_math.hpp"

namespace rb {

constexpr uint32_t kSiftMaxSlots = 128;   // a node's list: four blocks of 32 candidate bits
constexpr uint32_t kSiftGroupMax = 4;     // triangles per group
constexpr uint32_t kSiftMinLive = 4;      // fewer live triangles: the plain loop is already short
constexpr double kSiftAlphaMax = 1e-3;    // members' normals agree to this angle
constexpr double kSiftBoxGrow = 1.05;     // the union box is no larger than the largest member's by this factor (sum of extents)
// ChunkMargins' constants (rb_device_chunk.hpp; certified by tools/margin_certify.py): rb_kernels.hip checks that these are those
constexpr float kSiftKS = 24.0f * 5.9604645e-8f * 1.01f, kSiftKP = 12.0f * 5.9604645e-8f * 1.01f, kSiftKT = 11.0f * 5.9604645e-8f * 1.01f,
                kSiftKD = 16.0f * 5.9604645e-8f * 1.01f;
constexpr double kSiftEdgeMax = 1e9, kSiftSpMax = 1e12;   // a closed group's longest edge, a launch's Sp: beyond them nothing is rejected
constexpr double kSiftSlabUlps = 8.0;    // pass 1's slab values: their rounding in units of u (M + Sp), on top of KS (sift_region)

// One group: 64 B, one wave-uniform 16-dword load.  An always-pass group has cap = fk = +inf (and zero extents): the kernel's
// test `f <= kChunkFMax` fails for it whatever the ray.
struct alignas(16) SiftGroup {
    float c[3];      // box centre
    float fk;        // bound of |e1| |e2| / (0.95 N), times 1.00001 and the slack of the kernel's approximate reciprocal: f = fk / lb
    float h[3];      // half extents, rounded up
    float cap;       // the determinant-floor cap (pack_fac's), +inf where it is beyond the range the bounds are claimed for
    float n[3];      // cone axis times a lower bound of cos(alpha)
    float s;         // upper bound of sin(alpha) plus the rounding of the dot product: lb = |d . n| - s
    uint32_t first, count;   // slots [first, first + count) of the node's list
    uint32_t closed, _pad;   // 1: the group can reject
};
static_assert(sizeof(SiftGroup) == 64, "one s_load_dwordx16");

struct SiftTable {
    std::vector<SiftGroup> groups;
    uint32_t first = 0, end = 0;         // the node's list
    uint32_t block_ends = 0;             // byte b: groups [0, that) cover the slots of blocks 0..b (a group never straddles a block)
    uint32_t live = 0, closed = 0;       // live triangles, groups that can reject
    float tmn[3] = {0, 0, 0}, tmx[3] = {0, 0, 0};   // box of the closed groups' triangles
    double lhalf = 0.0;                  // half the largest sum of a closed group's extents (>= L / 2 of its triangles)
};

// per launch: the box a lane's origin is tested against, and Sp_max folded into the four margin constants
struct SiftRegion {
    float lo[3], hi[3];
    float kp, ks, kt, kd;
    float rmax;      // |reciprocal| up to which c r, o r and (h + mm) |r| stay finite for every c, o in the region and every mm in range
    bool on = false;
};

namespace sift {

inline bool finite3(const float v[3]) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

struct Item {
    bool closed = false, live = false;
    chunkmath::ChunkItem it{};
    double lo[3], hi[3];
};

inline Item make_item(const PrepTri& t, uint32_t slot) {
    Item m;
    m.live = t.valid != 0u;
    if (!m.live || !finite3(t.v0) || !finite3(t.e1) || !finite3(t.e2)) return m;
    rb_gpu_triangle g{};   // make_item subtracts v1 - v0 in f32: from 0 that is the prepared edge itself
    for (int a = 0; a < 3; ++a) g.v1[a] = t.e1[a], g.v2[a] = t.e2[a];
    chunkmath::make_item(g, slot, 0u, m.it);
    for (int a = 0; a < 3; ++a) {
        const double p0 = t.v0[a], p1 = double(t.v0[a]) + double(t.e1[a]), p2 = double(t.v0[a]) + double(t.e2[a]);
        m.lo[a] = chunkmath::dmin(p0, chunkmath::dmin(p1, p2));
        m.hi[a] = chunkmath::dmax(p0, chunkmath::dmax(p1, p2));
    }
    m.closed = m.it.has_normal && std::isfinite(m.it.fa_l) && std::isfinite(m.it.fa) && m.it.fa_l > 0.0;
    return m;
}

inline SiftGroup open_group(uint32_t first, uint32_t count) {
    SiftGroup g{};
    g.fk = g.cap = chunkmath::f_inf();
    g.first = first;
    g.count = count;
    return g;
}

inline double ext_sum(const double lo[3], const double hi[3]) { return (hi[0] - lo[0]) + (hi[1] - lo[1]) + (hi[2] - lo[2]); }

// the record of closed items [a, b) if they may form one group; false if they may not
inline bool close_group(const std::vector<Item>& items, uint32_t a, uint32_t b, uint32_t first_slot, SiftGroup& out) {
    double lo[3], hi[3], largest = 0.0;
    for (int k = 0; k < 3; ++k) lo[k] = items[a].lo[k], hi[k] = items[a].hi[k];
    double cap = 0, fa = 0, cap_l = 0, fa_l = 0;
    for (uint32_t i = a; i < b; ++i) {
        const Item& m = items[i];
        for (int k = 0; k < 3; ++k) lo[k] = chunkmath::dmin(lo[k], m.lo[k]), hi[k] = chunkmath::dmax(hi[k], m.hi[k]);
        largest = chunkmath::dmax(largest, ext_sum(m.lo, m.hi));
        cap = chunkmath::dmax(cap, m.it.cap), fa = chunkmath::dmax(fa, m.it.fa);
        cap_l = chunkmath::dmax(cap_l, m.it.cap_l), fa_l = chunkmath::dmax(fa_l, m.it.fa_l);
    }
    if (b - a > 1u && !(ext_sum(lo, hi) <= kSiftBoxGrow * largest)) return false;
    // E1-E7 are bounds on roundings: no intermediate of the reference's test may overflow.  Its largest is of the order |s| L^2,
    // so edges beyond kSiftEdgeMax (and, in sift_region, an Sp beyond kSiftSpMax) leave a group open: |s| L^2 <= 1e30.
    if (!(cap_l <= kSiftEdgeMax * kSiftEdgeMax * 1e6 * (1.0 + 1e-5))) return false;
    const chunkmath::DCone cone = chunkmath::cone_of([&](uint32_t i) -> const chunkmath::ChunkItem& { return items[a + i].it; }, b - a);
    if (!cone.valid || !(cone.alpha <= kSiftAlphaMax)) return false;
    // pack_fac's rule in f32: a triangle beyond the range the bounds are claimed for stores no cap, and its |cos| >= c0 bound with L^2
    const bool beyond = !(cap_l * (1.0 + 1e-6) <= 1.5e5);
    const double capv = beyond ? HUGE_VAL : cap * (1.0 + 1e-6), fav = beyond ? fa_l : fa;
    const double fk = fav * double(kFastGrazeCos) * 1.00001 * (1.0 + 2e-6);   // 2e-6: v_rcp_f32 is within 1 ulp, and the product's rounding
    if (!(fk <= 1.5e5)) return false;   // no ray can stay inside the bounds' range
    SiftGroup g{};
    for (int k = 0; k < 3; ++k) {
        const double mid = 0.5 * (lo[k] + hi[k]);
        g.c[k] = static_cast<float>(mid);
        const double half = chunkmath::dmax(hi[k] - double(g.c[k]), double(g.c[k]) - lo[k]);
        const double pad = half * (1.0 + 1e-6) + 1e-12 * std::fabs(mid) + 1e-37;   // the box's own rounding (sums in double: 2^-53)
        g.h[k] = chunkmath::f32_not_below(pad, half);
        if (!std::isfinite(g.c[k]) || !std::isfinite(g.h[k])) return false;
    }
    g.fk = chunkmath::f32_not_below(fk, fk);
    g.cap = std::isfinite(capv) ? chunkmath::f32_not_below(capv, capv) : chunkmath::f_inf();
    const double cos_a = std::cos(cone.alpha) * (1.0 - 1e-6) - 1e-7;
    for (int k = 0; k < 3; ++k) g.n[k] = static_cast<float>(cone.c[k] * cos_a);
    const double sin_a = std::sin(cone.alpha) * (1.0 + 1e-5) + 2e-6;   // 2e-6: the f32 dot product, |d| = 1 +- 4 u, n's own rounding
    g.s = chunkmath::f32_not_below(sin_a, sin_a);
    g.first = first_slot + a;
    g.count = b - a;
    g.closed = 1u;
    out = g;
    return true;
}

}  // namespace sift

// The groups of a node's list ptris[first, end) (slot order).  Grouping is a heuristic: neighbours merge while close_group
// agrees, open items (invalid, non-finite, no normal) merge with open items; no group crosses a block of 32 slots.
inline void build_sift_table(const PrepTri* ptris, uint32_t first, uint32_t end, SiftTable& tb) {
    tb = SiftTable{};
    tb.first = first, tb.end = end;
    if (end <= first || end - first > kSiftMaxSlots) return;
    const uint32_t n = end - first;
    std::vector<sift::Item> items(n);
    for (uint32_t i = 0; i < n; ++i) {
        items[i] = sift::make_item(ptris[first + i], first + i);
        tb.live += items[i].live ? 1u : 0u;
    }
    for (uint32_t i = 0; i < n; ++i) {   // closed: the triangle can form a group on its own
        SiftGroup alone;
        items[i].closed = items[i].closed && sift::close_group(items, i, i + 1u, first, alone);
    }
    bool any = false;
    uint32_t a = 0;
    while (a < n) {
        const uint32_t block_end = std::min(n, (a / 32u + 1u) * 32u);
        SiftGroup g = sift::open_group(first + a, 1u);
        uint32_t b = a + 1u;
        if (items[a].closed && sift::close_group(items, a, b, first, g)) {
            SiftGroup wider;
            while (b < block_end && b - a < kSiftGroupMax && items[b].closed && sift::close_group(items, a, b + 1u, first, wider)) g = wider, ++b;
        } else {
            g = sift::open_group(first + a, 1u);
            // an item that is closed but cannot form a group on its own stays open; open neighbours join it
            while (b < block_end && b - a < kSiftGroupMax && !items[b].closed) ++b;
            g.count = b - a;
        }
        if (g.closed) {
            tb.closed++;
            double sum = 0.0;
            for (int k = 0; k < 3; ++k) {
                const float lo = g.c[k] - g.h[k], hi = g.c[k] + g.h[k];
                const float lo_ = std::nextafter(lo, -chunkmath::f_inf()), hi_ = std::nextafter(hi, chunkmath::f_inf());
                tb.tmn[k] = any ? std::min(tb.tmn[k], lo_) : lo_;
                tb.tmx[k] = any ? std::max(tb.tmx[k], hi_) : hi_;
                sum += 2.0 * double(g.h[k]);
            }
            tb.lhalf = chunkmath::dmax(tb.lhalf, 0.5 * sum);
            any = true;
        }
        tb.groups.push_back(g);
        a = b;
    }
    // cumulative group counts at the end of each block of 32 slots
    uint32_t gi = 0;
    for (uint32_t blk = 0; blk < 4u; ++blk) {
        while (gi < tb.groups.size() && tb.groups[gi].first - first < (blk + 1u) * 32u) ++gi;
        tb.block_ends |= gi << (8u * blk);
    }
}

// Does a launch over this table sift?  Single node is the caller's business; here: enough live triangles, one group that can reject.
inline bool sift_pays(const SiftTable& tb) { return !tb.groups.empty() && tb.live >= kSiftMinLive && tb.closed >= 1u; }

// The origin region: the box of the closed groups' triangles and of `extra` (n_extra boxes as lo[3], hi[3]: the camera, the spheres),
// padded so that a hit point's own rounding stays inside; Sp_max = its diagonal + L_max / 2.  ks carries, beside ChunkMargins::KS, the
// rounding of pass 1's slab values: fma(c, inv, -(o inv)) with an approximate inv is off by at most 3 u M |inv| + 2 u Sp |inv|
// (M: the largest coordinate magnitude), taken as 8 u (M + Sp).
inline SiftRegion sift_region(const SiftTable& tb, const float (*extra)[6], uint32_t n_extra, float KP = kSiftKP, float KS = kSiftKS,
                              float KT = kSiftKT, float KD = kSiftKD) {
    SiftRegion r{};
    if (!sift_pays(tb)) return r;
    double lo[3], hi[3];
    for (int k = 0; k < 3; ++k) lo[k] = tb.tmn[k], hi[k] = tb.tmx[k];
    for (uint32_t i = 0; i < n_extra; ++i)
        for (int k = 0; k < 3; ++k) {
            if (!std::isfinite(extra[i][k]) || !std::isfinite(extra[i][3 + k])) return r;
            lo[k] = chunkmath::dmin(lo[k], extra[i][k]), hi[k] = chunkmath::dmax(hi[k], extra[i][3 + k]);
        }
    double m = 0.0, diag2 = 0.0;
    for (int k = 0; k < 3; ++k) m = chunkmath::dmax(m, chunkmath::dmax(std::fabs(lo[k]), std::fabs(hi[k])));
    const double pad = 1e-3 * chunkmath::dmax(m, chunkmath::dmax(hi[0] - lo[0], chunkmath::dmax(hi[1] - lo[1], hi[2] - lo[2]))) + 1e-30;
    for (int k = 0; k < 3; ++k) {
        const double l = lo[k] - pad, h = hi[k] + pad;
        r.lo[k] = std::nextafter(static_cast<float>(l), -chunkmath::f_inf());
        r.hi[k] = std::nextafter(static_cast<float>(h), chunkmath::f_inf());
        diag2 += (double(r.hi[k]) - double(r.lo[k])) * (double(r.hi[k]) - double(r.lo[k]));
        m = chunkmath::dmax(m, chunkmath::dmax(std::fabs(double(r.lo[k])), std::fabs(double(r.hi[k]))));
    }
    const double u = 5.9604645e-8;
    const double sp = 1.001 * (std::sqrt(diag2) + tb.lhalf);
    const double kp = sp * double(KP) * (1.0 + 1e-6), ks = (sp * double(KS) + kSiftSlabUlps * u * (m + sp)) * (1.0 + 1e-6);
    const double kt = sp * double(KT) * (1.0 + 1e-6), kd = sp * double(KD) * (1.0 + 1e-6);
    r.kp = chunkmath::f32_not_below(kp, kp), r.ks = chunkmath::f32_not_below(ks, ks);
    r.kt = chunkmath::f32_not_below(kt, kt), r.kd = chunkmath::f32_not_below(kd, kd);
    // pass 1 forms c r - o r -+ (h + mm) |r| with |c|, |o| <= M, h <= Sp, mm <= kp FMax + ks (f in range; beyond it the lane is a
    // candidate whatever the slab values): with |r| <= rmax every product and every sum of them is below 1e38 < FLT_MAX
    const double reach = 2.0 * m + sp + (kp * 1.5e5 + ks);
    r.rmax = static_cast<float>(1e38 / reach);
    if (double(r.rmax) * reach > 1e38) r.rmax = std::nextafter(r.rmax, 0.0f);
    r.on = sp <= kSiftSpMax && std::isfinite(r.rmax) && r.rmax > 0.0f && std::isfinite(r.kp) && std::isfinite(r.ks) && std::isfinite(r.kt) && std::isfinite(r.kd) && std::isfinite(r.lo[0]) &&
           std::isfinite(r.lo[1]) && std::isfinite(r.lo[2]) && std::isfinite(r.hi[0]) && std::isfinite(r.hi[1]) && std::isfinite(r.hi[2]);
    return r;
}

}  // namespace rb
