// rb_color_plan.hpp -- how a group of passes is cut into launches of the stream kernels, and how many colour parts those
// launches alternate between (dispatch in rb_runtime.cpp; DESIGN.md section 4, "Why two phases").  Plain arithmetic on
// integers: host code only, no HIP, so that a stand-alone program can exercise it (tests/test_color_plan.py).
#pragma once
#include <algorithm>
#include <cstdint>

namespace rb {

struct ColorPlan {
    uint32_t chunk = 0;   // passes per launch (the last launch of a group may be shorter); 0: the frame does not fit a launch
    uint32_t parts = 1;   // colour parts of per_pass * chunk items each: 1, or 2 with launch i writing part i % 2
    uint32_t launches(uint32_t n_passes) const { return chunk ? (n_passes + chunk - 1) / chunk : 0; }
    uint64_t floats(uint64_t per_pass) const { return per_pass * chunk * parts * 4ull; }   // one float4 per item
};

// per_pass: items (pixel, sample) of one pass, at least 1; n_passes: the group, at least 1; fixed_chunk: the caller's
// passes_per_launch (0: none); budget_items: items the colour buffer may hold (ignored when the caller fixed the chunk, as
// it always was).  A launch stays below 2^31 items: the kernels count items in 32 bits.
//  * The group fits one launch: one part, and nothing differs from a library without the second part.
//  * Otherwise the same budget is cut into two equal parts, so that a launch's colours can be accumulated while the next
//    launch traces into the other part: twice the launches of half the size, no more memory.  A caller's fixed chunk is
//    kept as given and gets two parts of that size -- the caller fixed the launch, not the memory.
//  * A budget whose half does not hold one pass keeps one part of one pass, as before.
inline ColorPlan plan_colors(uint64_t per_pass, uint32_t n_passes, uint32_t fixed_chunk, uint64_t budget_items) {
    ColorPlan pl;
    per_pass = std::max<uint64_t>(per_pass, 1);
    const uint64_t launch_cap = std::min<uint64_t>((1ull << 31) / per_pass, 0xFFFFFFFFull);   // passes a launch can count
    if (launch_cap == 0) return pl;
    const uint64_t want = fixed_chunk ? fixed_chunk : n_passes;
    const uint64_t whole = fixed_chunk ? launch_cap : std::min(launch_cap, std::max<uint64_t>(budget_items / per_pass, 1));
    if (std::min(want, whole) >= n_passes) {
        pl.chunk = n_passes;
        return pl;
    }
    const uint64_t half = fixed_chunk ? std::min(want, launch_cap) : std::min(launch_cap, (budget_items / 2) / per_pass);
    if (half == 0) {
        pl.chunk = static_cast<uint32_t>(std::min(want, whole));
        return pl;
    }
    pl.chunk = static_cast<uint32_t>(half);
    pl.parts = 2;
    return pl;
}

// the device could not give the plan's buffer: half the chunk, the parts as they are; false when there is nothing left to halve
inline bool halve(ColorPlan& pl) {
    if (pl.chunk <= 1) return false;
    pl.chunk = (pl.chunk + 1) / 2;
    return true;
}

}  // namespace rb
