// rb_lightmap.hip -- lightmap texels made on the device (rb_lightmap_surfels, rb_lightmap_resolve, rb_bake_lightmap; DESIGN.md
// section 17, the normative definition): the triangles of a mesh rasterised in uv space into an atlas, the owner of every texel,
// the surfel of every owned texel, and after the trace the resolve of the sums with its gutter fill.  Same numerics contract as
// rb_kernels.hip: every step one binary32 operation in the order written, no FMA contraction, correctly rounded /, so that
// renderbaby_amd/lightmap.py equals this file bit for bit.
//
// The cover pass deals its work in units of one (triangle, 8 x 8-texel tile of the atlas inside the triangle's box): a wall of
// two triangles over the whole atlas and a fixture of 68 768 triangles of a few texels each both fill their wavefronts.
//   k_lm_count    lane = triangle: texel space, validity, mesh filter, the box in tiles -> units per triangle
//   (scan)        rocPRIM exclusive scan of the counts; the host reads the total alone
//   k_lm_cover    wave = unit, lane = texel of the tile: atomicMin of the triangle index on every covered texel
//   k_lm_surfels  lane = texel: the owner's barycentrics from the same operations -> the 32-byte surfel
//   k_lm_resolve, k_lm_dilate   lane = texel: sum / weight, then the fill passes
#include <algorithm>
#include <utility>

#include <rocprim/device/device_scan.hpp>

#include "rb_device_common.hpp"

#pragma clang fp contract(off)

namespace rb {
namespace {

DEV bool lm_finite(float a) { return (__float_as_uint(a) & 0x7F800000u) != 0x7F800000u; }

// an edge with its ends in canonical order: two triangles that share it evaluate the same E and differ in the sign alone
struct LmEdge {
    float ax, ay, dx, dy;
    bool ordered;
};
DEV LmEdge lm_edge(float sx, float sy, float tx, float ty) {
    const bool ord = sx < tx || (sx == tx && sy <= ty);
    const float ax = ord ? sx : tx, ay = ord ? sy : ty, bx = ord ? tx : sx, by = ord ? ty : sy;
    return LmEdge{ax, ay, bx - ax, by - ay, ord};
}
DEV float lm_eval(const LmEdge& e, float px, float py) {
    const float v = e.dx * (py - e.ay) - e.dy * (px - e.ax);
    return e.ordered ? v : -v;
}

// what a triangle is to the atlas: its three edges, its area, its box in texels (x0 <= x1, y0 <= y1 when `any`)
struct LmTri {
    LmEdge bc, ca, ab;
    float area;
    uint32_t x0, x1, y0, y1;
    bool any;
};

DEV float lm_uv(const LmArgs& g, uint32_t i) { return i < g.n_uvs ? cptr(g.uvs)[i] : 0.0f; }

// One function for every kernel, so that a value has the same bits wherever it is made.  With a wave-uniform t every load
// here is a scalar load and the result lives in scalar registers.
DEV LmTri lm_setup(const LmArgs& g, uint32_t t) {
    LmTri r{};
    r.any = false;
    const v4u a = ((cu4p)g.ptris)[(size_t)t * 4u + 1u], b = ((cu4p)g.ptris)[(size_t)t * 4u + 2u];   // {e1, mesh_index}, {e2, valid}
    const uint32_t mesh_index = a.w, valid = b.w;
    if (valid == 0u || (g.mesh != RB_LIGHTMAP_ALL_MESHES && mesh_index != g.mesh)) return r;
    const v4u s = ((cu4p)g.pshade)[t];
    const float fw = (float)g.width, fh = (float)g.height;
    const float ax = lm_uv(g, s.x * 2u) * fw, ay = (1.0f - lm_uv(g, s.x * 2u + 1u)) * fh;
    const float bx = lm_uv(g, s.y * 2u) * fw, by = (1.0f - lm_uv(g, s.y * 2u + 1u)) * fh;
    const float cx = lm_uv(g, s.z * 2u) * fw, cy = (1.0f - lm_uv(g, s.z * 2u + 1u)) * fh;
    if (!(lm_finite(ax) && lm_finite(ay) && lm_finite(bx) && lm_finite(by) && lm_finite(cx) && lm_finite(cy))) return r;
    r.ab = lm_edge(ax, ay, bx, by);
    r.bc = lm_edge(bx, by, cx, cy);
    r.ca = lm_edge(cx, cy, ax, ay);
    r.area = lm_eval(r.ab, cx, cy);
    if (!lm_finite(r.area) || r.area == 0.0f) return r;
    const float lox = floorf(fminf(fminf(ax, bx), cx)), hix = floorf(fmaxf(fmaxf(ax, bx), cx));
    const float loy = floorf(fminf(fminf(ay, by), cy)), hiy = floorf(fmaxf(fmaxf(ay, by), cy));
    const float mx = (float)(g.width - 1u), my = (float)(g.height - 1u);
    if (hix < 0.0f || hiy < 0.0f || lox > mx || loy > my) return r;
    r.x0 = (uint32_t)fmaxf(lox, 0.0f);
    r.x1 = (uint32_t)fminf(hix, mx);
    r.y0 = (uint32_t)fmaxf(loy, 0.0f);
    r.y1 = (uint32_t)fminf(hiy, my);
    r.any = true;
    return r;
}

DEV uint32_t lm_tiles_x(const LmTri& r) { return r.x1 / kLmTile - r.x0 / kLmTile + 1u; }
DEV uint32_t lm_tiles_y(const LmTri& r) { return r.y1 / kLmTile - r.y0 / kLmTile + 1u; }

// all three on the triangle's side of zero; zero is inside for either winding
DEV bool lm_inside(float area, float w0, float w1, float w2) {
    return area > 0.0f ? (w0 >= 0.0f && w1 >= 0.0f && w2 >= 0.0f) : (w0 <= 0.0f && w1 <= 0.0f && w2 <= 0.0f);
}

// Every texel centre of the tile is outside edge e?  E is monotonic in P.x and in P.y separately -- each of its seven
// operations is, rounding included --, so over a rectangle of centres it takes its largest and its smallest value at a corner:
// the four corner values, made by lm_eval itself, decide for all 64 and never drop a covered texel.
DEV bool lm_tile_outside(const LmEdge& e, float area, float fx0, float fy0) {
    const float fx1 = fx0 + (float)(kLmTile - 1u), fy1 = fy0 + (float)(kLmTile - 1u);
    const float c0 = lm_eval(e, fx0, fy0), c1 = lm_eval(e, fx1, fy0), c2 = lm_eval(e, fx0, fy1), c3 = lm_eval(e, fx1, fy1);
    return area > 0.0f ? (c0 < 0.0f && c1 < 0.0f && c2 < 0.0f && c3 < 0.0f) : (c0 > 0.0f && c1 > 0.0f && c2 > 0.0f && c3 > 0.0f);
}

__global__ void __launch_bounds__(256) k_lm_iota(uint32_t* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) out[i] = i;
}

// ========================================================= k_lm_count ====
// lane = triangle; counts[n_tris] = 0, so that the exclusive scan of n_tris + 1 counts ends in the total
__global__ void __launch_bounds__(256) k_lm_count(const LmArgs g, unsigned long long* __restrict__ counts) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t > g.n_tris) return;
    unsigned long long c = 0ull;
    if (t < g.n_tris) {
        const LmTri r = lm_setup(g, t);
        if (r.any) c = (unsigned long long)lm_tiles_x(r) * lm_tiles_y(r);
    }
    counts[t] = c;
}

// ========================================================= k_lm_cover ====
// wave = unit `unit_base + 4 * block + wave-in-block`, lane = texel of the unit's tile.  The unit index is made wave-uniform
// for the compiler (readfirstlane), so the search of the scan, the triangle's record and everything derived from it are scalar.
__global__ void __launch_bounds__(256) k_lm_cover(const LmArgs g, const unsigned long long* __restrict__ scan, unsigned long long unit_base,
                                                  unsigned long long unit_end, uint32_t* __restrict__ owners) {
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    const unsigned long long unit = unit_base + (unsigned long long)blockIdx.x * 4ull + wave;
    if (unit >= unit_end) return;
    // the triangle whose units [scan[t], scan[t + 1]) hold `unit`: the last t with scan[t] <= unit (those before it with the same
    // scan value have no units)
    uint32_t lo = 0u, hi = g.n_tris;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (cptr(scan)[mid] <= unit) lo = mid;
        else hi = mid;
    }
    const uint32_t t = lo;
    const LmTri r = lm_setup(g, t);
    if (!r.any) return;   // (cannot be: the unit is one of its box's tiles)
    const uint32_t local = (uint32_t)(unit - cptr(scan)[t]), ntx = lm_tiles_x(r);
    const uint32_t ty = local / ntx, tx = local - ty * ntx;
    if (ty >= lm_tiles_y(r)) return;
    const uint32_t X0 = (r.x0 / kLmTile + tx) * kLmTile, Y0 = (r.y0 / kLmTile + ty) * kLmTile;
    const float fx0 = (float)X0 + 0.5f, fy0 = (float)Y0 + 0.5f;
    if (lm_tile_outside(r.bc, r.area, fx0, fy0) || lm_tile_outside(r.ca, r.area, fx0, fy0) || lm_tile_outside(r.ab, r.area, fx0, fy0)) return;
    const uint32_t x = X0 + (lane & 7u), y = Y0 + (lane >> 3);
    if (x < r.x0 || x > r.x1 || y < r.y0 || y > r.y1) return;   // the box lies inside the atlas
    const float px = (float)x + 0.5f, py = (float)y + 0.5f;
    const float w0 = lm_eval(r.bc, px, py), w1 = lm_eval(r.ca, px, py), w2 = lm_eval(r.ab, px, py);
    if (!lm_inside(r.area, w0, w1, w2)) return;
    // u32 minimum: exact and order-free, so relaxed at agent scope is all it needs (as the box atomics of rb_build.hip)
    (void)__hip_atomic_fetch_min(&owners[(size_t)y * g.width + x], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ========================================================= k_lm_surfels ====
// lane = texel.  w1, w2 and area are lm_setup's and lm_eval's again: the same operations on the same operands as in k_lm_cover.
__global__ void __launch_bounds__(256) k_lm_surfels(const LmArgs g, const uint32_t* __restrict__ owners, rb_surfel* __restrict__ surfels) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t n = g.width * g.height;
    if (i >= n) return;
    const uint32_t t = owners[i];
    v4f s0 = {0.0f, 0.0f, 0.0f, 0.0f}, s1 = {0.0f, 0.0f, 0.0f, 0.0f};
    if (t < g.n_tris) {
        const LmTri r = lm_setup(g, t);
        const uint32_t y = i / g.width, x = i - y * g.width;
        const float px = (float)x + 0.5f, py = (float)y + 0.5f;
        const float u = lm_eval(r.ca, px, py) / r.area, v = lm_eval(r.ab, px, py) / r.area;
        const v4f* const rec = reinterpret_cast<const v4f*>(g.ptris) + (size_t)t * 4u;
        const v4f v0 = rec[0], e1 = rec[1], e2 = rec[2], nn = rec[3];
        s0.x = (v0.x + u * e1.x) + v * e2.x;
        s0.y = (v0.y + u * e1.y) + v * e2.y;
        s0.z = (v0.z + u * e1.z) + v * e2.z;
        const bool flip = (g.flags & RB_LIGHTMAP_FLIP) != 0u;
        s1.x = flip ? -nn.x : nn.x;
        s1.y = flip ? -nn.y : nn.y;
        s1.z = flip ? -nn.z : nn.z;
    }
    v4f* const out = reinterpret_cast<v4f*>(surfels) + (size_t)i * 2u;
    out[0] = s0;
    out[1] = s1;
}

// ========================================================= k_lm_resolve, k_lm_dilate ====
__global__ void __launch_bounds__(256) k_lm_resolve(const rb_radiance* __restrict__ sums, uint32_t n, float* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const v4f s = reinterpret_cast<const v4f*>(sums)[i];
    v4f r = {0.0f, 0.0f, 0.0f, 0.0f};
    if (s.w > 0.0f) {
        r.x = s.x / s.w;
        r.y = s.y / s.w;
        r.z = s.z / s.w;
        r.w = 1.0f;
    }
    reinterpret_cast<v4f*>(out)[i] = r;
}

// one pass: reads `in` alone, writes every texel of `out`
__global__ void __launch_bounds__(256) k_lm_dilate(const float* __restrict__ in, uint32_t width, uint32_t height, float* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= width * height) return;
    const v4f* const src = reinterpret_cast<const v4f*>(in);
    v4f c = src[i];
    if (c.w == 0.0f) {
        const uint32_t y = i / width, x = i - y * width;
        float sr = 0.0f, sg = 0.0f, sb = 0.0f;
        uint32_t cnt = 0u;
        for (int dy = -1; dy <= 1; dy++)
            for (int dx = -1; dx <= 1; dx++) {
                if (dx == 0 && dy == 0) continue;
                const uint32_t nx = x + (uint32_t)dx, ny = y + (uint32_t)dy;   // (wraps past the atlas for -1 at 0)
                if (nx >= width || ny >= height) continue;
                const v4f q = src[(size_t)ny * width + nx];
                if (q.w != 0.0f) {
                    sr = sr + q.x;
                    sg = sg + q.y;
                    sb = sb + q.z;
                    cnt++;
                }
            }
        if (cnt > 0u) {
            const float fc = (float)cnt;
            c.x = sr / fc;
            c.y = sg / fc;
            c.z = sb / fc;
            c.w = 2.0f;
        }
    }
    reinterpret_cast<v4f*>(out)[i] = c;
}

size_t lm_align(size_t b) { return (b + 255u) & ~size_t(255); }

hipError_t lm_scan(void* temp, size_t& temp_bytes, unsigned long long* counts, unsigned long long* scan, uint32_t n, hipStream_t stream) {
    return rocprim::exclusive_scan(temp, temp_bytes, counts, scan, 0ull, n, rocprim::plus<unsigned long long>(), stream);
}

}  // namespace

int launch_lightmap_iota(uint32_t* out, uint32_t n, void* stream_) {
    if (n == 0u) return 0;
    hipLaunchKernelGGL(k_lm_iota, dim3((n + 255u) / 256u), dim3(256), 0, static_cast<hipStream_t>(stream_), out, n);
    return (int)hipGetLastError();
}

// counts | scan | rocPRIM's temporary storage, each 256-byte aligned
size_t lightmap_work_bytes(uint32_t n_tris) {
    size_t temp = 0;
    if (lm_scan(nullptr, temp, nullptr, nullptr, n_tris + 1u, nullptr) != hipSuccess) temp = 0;
    return 2u * lm_align(8u * ((size_t)n_tris + 1u)) + lm_align(temp) + 256u;
}

int lightmap_surfels(const LmArgs& g, rb_surfel* surfels, uint32_t* owners, void* work, uint64_t piece_units, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const uint64_t n = (uint64_t)g.width * g.height;
    if (n == 0u || n > 0x7FFFFFFFull - 63ull || surfels == nullptr || owners == nullptr) return (int)hipErrorInvalidValue;
    if (g.n_tris > 0x7FFFFFFFu - 63u) return (int)hipErrorInvalidValue;
    hipError_t st = hipMemsetAsync(owners, 0xFF, n * sizeof(uint32_t), stream);
    if (st != hipSuccess) return (int)st;
    if (g.n_tris > 0u) {
        if (work == nullptr || g.ptris == nullptr || g.pshade == nullptr) return (int)hipErrorInvalidValue;
        const uint32_t m = g.n_tris + 1u;
        char* const base = static_cast<char*>(work);
        unsigned long long* const counts = reinterpret_cast<unsigned long long*>(base);
        unsigned long long* const scan = reinterpret_cast<unsigned long long*>(base + lm_align(8u * (size_t)m));
        void* const temp = base + 2u * lm_align(8u * (size_t)m);
        size_t temp_bytes = 0;
        st = lm_scan(nullptr, temp_bytes, counts, scan, m, stream);
        if (st != hipSuccess) return (int)st;
        hipLaunchKernelGGL(k_lm_count, dim3((m + 255u) / 256u), dim3(256), 0, stream, g, counts);
        st = hipGetLastError();
        if (st == hipSuccess) st = lm_scan(temp, temp_bytes, counts, scan, m, stream);
        unsigned long long total = 0ull;
        if (st == hipSuccess) st = hipMemcpyAsync(&total, scan + g.n_tris, 8, hipMemcpyDeviceToHost, stream);
        if (st == hipSuccess) st = hipStreamSynchronize(stream);
        if (st != hipSuccess) return (int)st;
        // at most 2^31 / 64 tiles of the atlas for each of at most 2^31 triangles: the total fits 64 bits with room to spare
        const uint64_t piece = piece_units ? std::min<uint64_t>(piece_units, 1ull << 30) : kLmPieceUnits;
        for (uint64_t done = 0; done < total; done += piece) {
            const uint64_t units = std::min<uint64_t>(piece, total - done);
            hipLaunchKernelGGL(k_lm_cover, dim3((uint32_t)((units + 3u) / 4u)), dim3(256), 0, stream, g, scan, done, done + units, owners);
            st = hipGetLastError();
            if (st != hipSuccess) return (int)st;
        }
    }
    hipLaunchKernelGGL(k_lm_surfels, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, stream, g, owners, surfels);
    return (int)hipGetLastError();
}

int launch_lightmap_resolve(const rb_radiance* sums, uint32_t width, uint32_t height, uint32_t dilate, float* out, float* tmp, void* stream_) {
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const uint64_t n = (uint64_t)width * height;
    if (n == 0u || n > 0x7FFFFFFFull - 63ull || sums == nullptr || out == nullptr || (dilate > 0u && tmp == nullptr)) return (int)hipErrorInvalidValue;
    const dim3 grid((uint32_t)((n + 255u) / 256u));
    float* cur = (dilate & 1u) ? tmp : out;   // so that the last pass writes `out`
    float* nxt = (dilate & 1u) ? out : tmp;
    hipLaunchKernelGGL(k_lm_resolve, grid, dim3(256), 0, stream, sums, (uint32_t)n, cur);
    hipError_t st = hipGetLastError();
    for (uint32_t k = 0; k < dilate && st == hipSuccess; k++) {
        hipLaunchKernelGGL(k_lm_dilate, grid, dim3(256), 0, stream, cur, width, height, nxt);
        st = hipGetLastError();
        std::swap(cur, nxt);
    }
    return (int)st;
}

}  // namespace rb
