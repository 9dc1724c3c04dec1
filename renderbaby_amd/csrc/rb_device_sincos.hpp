// rb_device_sincos.hpp -- what the device's ray generators share (rb_camera.hip, rb_hemisphere.hip, rb_probe.hip): sincos_turn,
// their fixed polynomial sine and cosine, a lane's item in the two orders of whole items, the store of
// a record and the lanes of a launch.  Its includer keeps floating-point contraction off.
#pragma once
#include "rb_device_math.hpp"

#pragma clang fp contract(off)

namespace rb {
namespace {

// sin and cos of pi * s for s in [-1, 1] (section 15.3): q = the nearest quarter turn, r = s - q / 2 exactly, x = r * (float)pi
// with |x| <= pi / 4, the two Taylor polynomials in Horner form -- one multiply, then one add per step --, the result by the
// quadrant q mod 4.  Within 2^-22 of the true values; the coefficients are the binary64 quotients rounded to binary32.
struct SinCos {
    float s, c;
};
DEV SinCos sincos_turn(float s) {
    const float q = __builtin_rintf(2.0f * s);
    const float r = s - 0.5f * q;
    const float x = r * 3.14159274101257324f;
    const float x2 = x * x;
    float ps = (float)(1.0 / 362880.0);
    ps = ps * x2 + (float)(-1.0 / 5040.0);
    ps = ps * x2 + (float)(1.0 / 120.0);
    ps = ps * x2 + (float)(-1.0 / 6.0);
    ps = ps * x2 + 1.0f;
    const float sn = x * ps;
    float pc = (float)(1.0 / 40320.0);
    pc = pc * x2 + (float)(-1.0 / 720.0);
    pc = pc * x2 + (float)(1.0 / 24.0);
    pc = pc * x2 + (float)(-1.0 / 2.0);
    pc = pc * x2 + 1.0f;
    const uint32_t quad = (uint32_t)(int)q & 3u;
    SinCos o;
    o.s = quad == 0u ? sn : quad == 1u ? pc : quad == 2u ? -sn : -pc;
    o.c = quad == 0u ? pc : quad == 1u ? -sn : quad == 2u ? -pc : sn;
    return o;
}

// Lane t's item of a piece of `samples`-sample items (surfels, probes).  Item order (the trace's scratch): t = (block * samples +
// sample) * 64 + item-in-block, block = 64 consecutive items of the piece -- the order the k_cam kernels hand items out in, so a
// wave's 64 records are one contiguous 2 KiB.  Linear order: t = item-in-piece * samples + sample.  The caller drops
// idx >= n: the padding of the last block, and the lanes behind the last item.
struct GenItem {
    uint32_t smp, idx;
};
DEV GenItem gen_item(uint32_t t, uint32_t S, uint32_t linear) {
    GenItem it;
    if (linear != 0u) {
        it.idx = t / S;
        it.smp = t - it.idx * S;
    } else {
        const uint32_t row = t >> 6, blk = row / S;
        it.smp = row - blk * S;
        it.idx = blk * 64u + (t & 63u);
    }
    return it;
}

// record t of a generator: {origin, seed after the generator's draws}, {direction, 0} -- or, with `seeds`, the seed beside the
// record, whose fourth word is then 0
DEV void store_record(rb_ray* recs, uint32_t* seeds, uint32_t t, f3 o, f3 d, uint32_t seed) {
    const bool beside = seeds != nullptr;
    const v4f r0 = {o.x, o.y, o.z, __uint_as_float(beside ? 0u : seed)}, r1 = {d.x, d.y, d.z, 0.0f};
    v4f* const rec = reinterpret_cast<v4f*>(recs) + (size_t)t * 2u;
    rec[0] = r0;
    rec[1] = r1;
    if (beside) seeds[t] = seed;
}

// host: the lanes of one launch over n whole items in gen_item's two orders (item order: n rounded up to whole blocks of 64),
// or 0 where they pass 2^31 - 1
inline uint64_t gen_lanes(uint32_t n, uint32_t samples, uint32_t linear) {
    const uint64_t lanes = linear != 0u ? (uint64_t)n * samples : (((uint64_t)n + 63u) / 64u) * 64u * samples;
    return lanes > 0x7FFFFFFFull ? 0ull : lanes;
}

}  // namespace
}  // namespace rb
