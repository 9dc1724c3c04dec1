"""The filter of DESIGN.md section 13.1 once more, as plain loops over pixels and taps, written from the text and sharing
nothing with renderbaby_amd/denoise.py: no shifted arrays, no masks, one np.float32 per operation.  It is slow (a 20 x 24 frame
takes about a second) and it counts what it meets, so that a test can prove from the counters that a case occurred.

Below it: the frames with degenerate guide and colour values that tests/test_denoise_scalar.py (numpy model against these loops)
and tests/test_gpu_denoise_edges.py (device against the numpy model) share.  DESIGN.md section 13.5 has the tables.
"""
import numpy as np

from renderbaby_amd import abi

f32 = np.float32
TINY = f32(2.0 ** -126)   # the smallest normal binary32
H = (f32(0.375), f32(0.25), f32(0.0625))


def _subnormal(v):
    a = abs(v)
    return a > 0 and a < TINY


def filter_scalar(color, guides, params):
    """(out, counters): the linear vec4 (h, w, 4) float32 of section 13.1, and
    counters = {"prepare": {"nan_generated"}, "finish": {"nan_generated"}, "iterations": [one dict per iteration]} with
      fallback            live pixels whose wsum was 0 (r' = r), fallback_at their (y, x)
      zero_w              accepted taps with w == 0
      subnormal_w         accepted taps with a subnormal w
      class_skipped       taps inside the frame skipped because cls_q != cls_p
      frame_skipped       taps outside the frame
      subnormal_results   components of r' that are subnormal
      nan_generated       operations whose result is a NaN though no operand is one"""
    c = np.asarray(color, dtype=f32)
    g = np.asarray(guides, dtype=abi.GUIDE)
    h, w = g.shape
    iterations, npow = int(params["iterations"]), int(params["normal_power_log2"])
    sigma_depth, sigma_color, floor = f32(params["sigma_depth"]), f32(params["sigma_color"]), f32(params["albedo_floor"])
    nan = [0]

    def seen(r, a, b):
        if r != r and a == a and b == b:
            nan[0] += 1
        return r

    def add(a, b):
        return seen(f32(a + b), a, b)

    def sub(a, b):
        return seen(f32(a - b), a, b)

    def mul(a, b):
        return seen(f32(a * b), a, b)

    def div(a, b):
        return seen(f32(a / b), a, b)

    def gt(a, b):   # "max(a, b)" of section 13.1
        return a if a > b else b

    def dot(a, b):
        return add(add(mul(a[0], b[0]), mul(a[1], b[1])), mul(a[2], b[2]))

    def took():
        n, nan[0] = nan[0], 0
        return n

    counters = {"prepare": {}, "iterations": [], "finish": {}}
    with np.errstate(all="ignore"):
        # ---- prepare
        cls = [[int(g["cls"][y, x]) if all(np.isfinite(c[y, x, k]) for k in range(3)) else 0 for x in range(w)] for y in range(h)]
        m = [[[gt(f32(g["albedo"][y, x, k]), floor) for k in range(3)] for x in range(w)] for y in range(h)]
        r = [[[f32(c[y, x, k]) for k in range(3)] for x in range(w)] for y in range(h)]
        if iterations > 0:
            for y in range(h):
                for x in range(w):
                    if cls[y][x] != 0:
                        r[y][x] = [div(r[y][x][k], m[y][x][k]) for k in range(3)]
        counters["prepare"]["nan_generated"] = took()
        n = [[[f32(v) for v in g["normal"][y, x]] for x in range(w)] for y in range(h)]
        pos = [[[f32(v) for v in g["pos"][y, x]] for x in range(w)] for y in range(h)]
        # ---- iterations
        for i in range(iterations):
            s = 1 << i
            sigma_i = mul(sigma_color, f32(2.0 ** -i))
            sigma2 = mul(sigma_i, sigma_i)
            k_ = dict(fallback=0, fallback_at=[], zero_w=0, subnormal_w=0, class_skipped=0, frame_skipped=0, subnormal_results=0)
            new = [[list(px) for px in row] for row in r]
            for y in range(h):
                for x in range(w):
                    if cls[y][x] == 0:
                        continue
                    r_p, n_p, pos_p = r[y][x], n[y][x], pos[y][x]
                    total, wsum = [f32(0), f32(0), f32(0)], f32(0)
                    den = mul(sigma_depth, f32(g["t"][y, x]))
                    for dy in range(-2, 3):
                        for dx in range(-2, 3):
                            qy, qx = y + s * dy, x + s * dx
                            if qy < 0 or qy >= h or qx < 0 or qx >= w:
                                k_["frame_skipped"] += 1
                                continue
                            if cls[qy][qx] != cls[y][x]:
                                k_["class_skipped"] += 1
                                continue
                            r_q, n_q, pos_q = r[qy][qx], n[qy][qx], pos[qy][qx]
                            k = f32(H[abs(dx)] * H[abs(dy)])
                            w_n = gt(dot(n_p, n_q), f32(0))
                            for _ in range(npow):
                                w_n = mul(w_n, w_n)
                            e = [sub(pos_q[j], pos_p[j]) for j in range(3)]
                            w_z = gt(sub(f32(1), div(f32(abs(dot(n_p, e))), den)), f32(0))
                            wt = mul(mul(k, w_n), w_z)
                            if sigma_color > 0:
                                d = [sub(r_q[j], r_p[j]) for j in range(3)]
                                w_c = div(f32(1), add(f32(1), div(dot(d, d), sigma2)))
                                wt = mul(wt, w_c)
                            if wt == 0:
                                k_["zero_w"] += 1
                            elif _subnormal(wt):
                                k_["subnormal_w"] += 1
                            total = [add(total[j], mul(wt, r_q[j])) for j in range(3)]
                            wsum = add(wsum, wt)
                    if wsum != 0:
                        new[y][x] = [div(total[j], wsum) for j in range(3)]
                        k_["subnormal_results"] += sum(1 for v in new[y][x] if _subnormal(v))
                    else:
                        k_["fallback"] += 1
                        k_["fallback_at"].append((y, x))
            r = new
            k_["nan_generated"] = took()
            counters["iterations"].append(k_)
        # ---- finish
        out = np.empty((h, w, 4), dtype=f32)
        for y in range(h):
            for x in range(w):
                px = r[y][x]
                if iterations > 0 and cls[y][x] != 0:
                    px = [mul(px[k], m[y][x][k]) for k in range(3)]
                out[y, x, :3] = px
                out[y, x, 3] = 1
        counters["finish"]["nan_generated"] = took()
    return out, counters


# ---- frames with hazards
NAN, INF = float("nan"), float("inf")
# planted at 1 % of a frame, none of these makes the filter produce a non-finite word at a live pixel of finite colour
QUIET = {"normal": (0.0, -0.0, NAN, 1e-39, 1e-45),
         "t": (0.0, NAN, INF, -INF, -1.0, 1e-39, 3e38),
         "pos": (NAN, INF, -INF, 1e-39, 3e38),
         "albedo": (-1.0, NAN, 0.0, -0.0, 1e-39, -INF),
         "color": (-1.0, 1e-39, -0.0, 1e20),
         "cls": (7, 0x80000000, 0x7FC00000)}       # class words outside {0, GROUND, TRIANGLE, SPHERE}: the caller's to choose
PASS_THROUGH = (NAN, INF, -INF)                    # colour values that turn their pixel into class 0
# one such pixel makes NaN for its neighbours: these go one pixel to a frame
LOUD = (("normal", 1e20), ("normal", INF), ("t", -0.0), ("albedo", INF), ("color", 3e38), ("color", -3e38))


def benign(h, w, seed):
    """colour and guides of a well-behaved frame: the three filterable classes meeting at edges, unit normals up to 25 degrees
    apart within a surface, positions near tilted planes, t >= 4, albedo in [0, 1) with a good share below the default floor,
    a few class 0 islands, every colour finite and positive"""
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[0:h, 0:w]
    g = np.zeros((h, w), dtype=abi.GUIDE)
    region = ((xx * 3) // w + (yy * 2) // h) % 3
    g["cls"] = np.array([abi.HIT_GROUND, abi.HIT_TRIANGLE, abi.HIT_SPHERE], np.uint32)[region]
    nrm = np.array([[0, 1, 0], [0, 0, 1], [0.6, 0, 0.8]], f32)[region] + rng.normal(0, 0.15, (h, w, 3)).astype(f32)
    g["normal"] = (nrm / np.sqrt((nrm * nrm).sum(-1, keepdims=True), dtype=f32)).astype(f32)
    g["t"] = (f32(4.0) + f32(0.01) * xx + f32(0.02) * yy + region).astype(f32)
    g["pos"] = np.stack([f32(0.02) * xx, f32(0.03) * region + f32(0.0005) * rng.random((h, w)), f32(-0.02) * yy], -1).astype(f32)
    g["albedo"] = (rng.random((h, w, 3)) ** 3).astype(f32)
    signal = np.array([[0.9, 0.5, 0.2], [0.1, 0.4, 0.8], [2.5, 2.0, 0.3]], f32)[region]
    c = (signal * g["albedo"] + rng.gamma(0.5, 0.4, (h, w, 3)) + 1e-3).astype(f32)
    if h * w >= 12:
        g["cls"][rng.random((h, w)) < 0.04] = 0
    return c, g


def plant(c, g, field, value, where):
    """`value` into every component of `field` at the pixels of the boolean map `where`, in place; a non-finite colour into ONE
    channel, another from pixel to pixel (the other two stay finite: a pass-through pixel must keep them as they are)"""
    if field == "color" and not np.isfinite(value):
        ys, xs = np.nonzero(where)
        c[ys, xs, np.arange(len(ys)) % 3] = f32(value)
    elif field == "color":
        c[where] = f32(value)
    elif field == "cls":
        g["cls"][where] = np.uint32(value)
    else:
        g[field][where] = f32(value)


def spots(h, w, seed, share=0.01, allowed=None):
    """a boolean map with about `share` of the pixels set, at least one; only pixels of `allowed` if that is given and not empty"""
    rng = np.random.Generator(np.random.PCG64(seed + 1000003))
    at = rng.random((h, w)) < share
    at[rng.integers(0, h), rng.integers(0, w)] = True
    if allowed is not None and allowed.any():
        at &= allowed
        if not at.any():
            ys, xs = np.nonzero(allowed)
            k = rng.integers(0, len(ys))
            at[ys[k], xs[k]] = True
    return at


def frame_with(field, value, h=37, w=53, seed=11):
    """(colour, guides, planted): benign(h, w, seed) with `value` in `field` at about 1 % of the pixels"""
    c, g = benign(h, w, seed)
    at = spots(h, w, seed)
    plant(c, g, field, value, at)
    return c, g, at


def frame_with_everything(h, w, seed=12, share=0.01):
    """(colour, guides, planted): every value of QUIET and PASS_THROUGH, each at its own `share` of the pixels (a pixel may get
    several); planted[field] is the map of the pixels where that field was touched.  One pair of quiet values is loud together:
    t = -1 makes den negative, and a neighbour whose position is +-inf or 3e38 then gives w_z = 1 - inf / den = +inf.  The class
    words go in first, t = -1 then only into GROUND pixels and those positions only into others, so the two never meet in a tap."""
    c, g = benign(h, w, seed)
    planted = {}
    k = 0
    order = ["cls"] + [f for f in QUIET if f != "cls"]
    for field, values in [(f, QUIET[f]) for f in order] + [("color", PASS_THROUGH)]:
        for v in values:
            k += 1
            allowed = None
            if field == "t" and v == -1.0:
                allowed = g["cls"] == abi.HIT_GROUND
            elif field == "pos" and abs(v) > 1e38:
                allowed = g["cls"] != abi.HIT_GROUND
            at = spots(h, w, seed + 7919 * k, share, allowed)
            plant(c, g, field, v, at)
            planted[field] = planted.get(field, np.zeros((h, w), bool)) | at
    return c, g, planted


def loud_frame(field, value, h=33, w=35, seed=13):
    """(colour, guides, (y, x)): a benign frame without class 0 islands around the middle, one loud value at one live pixel
    near the middle"""
    c, g = benign(h, w, seed)
    y, x = h // 2, w // 2 - 1
    g["cls"][y - 4:y + 5, x - 4:x + 5] = g["cls"][y, x] if g["cls"][y, x] != 0 else abi.HIT_TRIANGLE
    at = np.zeros((h, w), bool)
    at[y, x] = True
    plant(c, g, field, value, at)
    return c, g, (y, x)


def subnormal_weight_frame(h=37, w=53, seed=14):
    """normals at a dot of 0.90 to 0.93 to their neighbours AND to themselves (their squared length is in that range, their
    directions agree to a degree): with normal_power_log2 = 10, w_n = dot^1024 lies between 1e-47 and 6e-33 at every tap, the
    centre's included -- across the subnormal range (1.4e-45 to 1.2e-38), under it and above it.  No large centre weight hides
    the small ones: many a pixel's wsum is subnormal itself, or 0.  One class, flat positions: nothing else takes weight away."""
    c, g = benign(h, w, seed)
    rng = np.random.Generator(np.random.PCG64(seed))
    g["cls"] = abi.HIT_TRIANGLE
    g["pos"][..., 1] = 0
    length = np.sqrt(rng.uniform(0.90, 0.93, (h, w)))
    tilt = rng.normal(0, 0.01, (h, w, 2))
    g["normal"] = (np.stack([tilt[..., 0], np.ones((h, w)), tilt[..., 1]], -1) * length[..., None]).astype(f32)
    return c, g


def subnormal_color_frame(h=37, w=53, seed=15):
    """a benign frame with colours scaled by 2^-130: w * r_q, the sums and sum / wsum have subnormal operands and results"""
    c, g = benign(h, w, seed)
    return (c * f32(2.0 ** -130)).astype(f32), g
