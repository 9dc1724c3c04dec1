"""Synthetic inputs of the temporal reprojection with expectations written by hand, shared by the model's
tests (test_reproject_model.py) and the device's (test_gpu_reproject.py).

The view looks along +z from (0, 0, -1) with right = x, up = y and dyadic cx, cy, sx, sy; every surface point lies on the plane
z = 0, so that e.z = 1, a / z = a, and X = cx - a * sx comes out exact for dyadic a.  Colours are small integers and albedos
powers of two: every product, quotient and sum of the definition is exact, and an expectation is a few lines of arithmetic.
"""
import numpy as np

from renderbaby_amd import abi, temporal

f32 = np.float32
W, H = 8, 4
NONE = np.zeros(4, f32)


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def flat_view(w=W, h=H, cam_x=0.0):
    """pos (cam_x, 0, -1); cx = (w - 1) / 2, sx = w / 2 (dyadic for the sizes used), the same for y"""
    v = np.zeros((), dtype=abi.VIEW)
    v["pos"], v["right"], v["up"], v["fwd"] = (cam_x, 0, -1), (1, 0, 0), (0, 1, 0), (0, 0, 1)
    v["cx"], v["cy"], v["sx"], v["sy"] = (w - 1) * 0.5, (h - 1) * 0.5, w * 0.5, h * 0.5
    return v


def flat_guides(view, w=W, h=H, shift_x=0.0, shift_y=0.0, depth=1.0, cls=abi.HIT_GROUND, albedo=0.5):
    """guides whose pixel (X, Y) projects to (X + shift_x, Y + shift_y) under `view`: points on the plane at `depth` in front of
    the view, normal towards it, t = depth"""
    g = np.zeros((h, w), dtype=abi.GUIDE)
    yy, xx = np.mgrid[0:h, 0:w]
    a = (f32(view["cx"]) - (xx + shift_x)) * depth / f32(view["sx"])
    b = (f32(view["cy"]) - (yy + shift_y)) * depth / f32(view["sy"])
    g["pos"] = np.stack([a + f32(view["pos"][0]), b + f32(view["pos"][1]), np.full_like(a, depth) + f32(view["pos"][2])], -1).astype(f32)
    g["normal"], g["t"], g["cls"], g["albedo"] = (0, 0, -1), depth, cls, albedo
    return g


def prev_frame(w=W, h=H):
    """records with small integer colours, all different, and counts 1 .. 4"""
    yy, xx = np.mgrid[0:h, 0:w]
    p = np.empty((h, w, 4), f32)
    p[..., 0], p[..., 1], p[..., 2] = 1 + xx + w * yy, 2 * (xx + 1), 64 - yy
    p[..., 3] = 1 + (xx + yy) % 4
    return p


def shifted(prev, dx):
    """prev moved so that out[:, x] = prev[:, x + dx], NONE where x + dx leaves the frame"""
    out = np.zeros_like(prev)
    w = prev.shape[1]
    if dx >= 0:
        out[:, :w - dx] = prev[:, dx:]
    else:
        out[:, -dx:] = prev[:, :w + dx]
    return out


def exact_cases():
    """(name, prev4, prev_guides, view, cur_guides, params, expected history) -- expected by hand"""
    v = flat_view()
    prev, pg = prev_frame(), flat_guides(v)
    p = temporal.params(max_history=64.0)
    cases = []
    # a shift by whole pixels: the previous frame shifted, count included, NONE in the uncovered columns
    for dx in (1, -1, 3):
        cases.append((f"whole pixel {dx:+d}", prev, pg, v, flat_guides(v, shift_x=dx), p, shifted(prev, dx)))
    # half a pixel: the exact mean of two neighbours; in the last column the right tap is outside, the left one alone remains
    want = np.zeros_like(prev)
    want[:, :-1] = (prev[:, :-1] + prev[:, 1:]) * f32(0.5)
    want[:, -1] = prev[:, -1]
    cases.append(("half pixel", prev, pg, v, flat_guides(v, shift_x=0.5), p, want))
    # the same downwards
    want = np.zeros_like(prev)
    want[:-1] = (prev[:-1] + prev[1:]) * f32(0.5)
    want[-1] = prev[-1]
    cases.append(("half pixel in y", prev, pg, v, flat_guides(v, shift_y=0.5), p, want))
    # X = -0.5 in column 0: pixel 0 alone, renormalised; the other columns the mean of their neighbours
    want = np.zeros_like(prev)
    want[:, 1:] = (prev[:, :-1] + prev[:, 1:]) * f32(0.5)
    want[:, 0] = prev[:, 0]
    cases.append(("X = -0.5", prev, pg, v, flat_guides(v, shift_x=-0.5), p, want))
    # X = -1 (column 0 of a shift by -1) and X = w (the last column of +1) are in the whole-pixel cases; here every column
    cases.append(("X = -1 everywhere", prev, pg, v, flat_guides(v, shift_x=-1.0 - np.arange(W)[None, :]), p, np.zeros_like(prev)))
    cases.append(("X = w everywhere", prev, pg, v, flat_guides(v, shift_x=float(W) - np.arange(W)[None, :]), p, np.zeros_like(prev)))
    # z = 0, z < 0, NaN in pos, class 0: NONE; the rest of the frame as without them
    cg = flat_guides(v)
    want = prev.copy()
    cg["pos"][0, 0, 2], cg["pos"][1, 1, 2], cg["pos"][2, 2, 0], cg["pos"][3, 3, 1], cg["pos"][0, 5, 2] = -1.0, -3.0, np.nan, np.nan, np.nan
    cg["cls"][1, 6] = 0
    for y, x in ((0, 0), (1, 1), (2, 2), (3, 3), (0, 5), (1, 6)):
        want[y, x] = 0
    cases.append(("z = 0, z < 0, NaN, class 0", prev, pg, v, cg, p, want))
    # max_history caps the count, and only the count
    big = prev.copy()
    big[..., 3] = 100
    want = big.copy()
    want[..., 3] = 32
    cases.append(("max_history", big, pg, v, flat_guides(v), temporal.default_params(), want))
    # demodulation by the previous albedo, remodulation by the current one
    pg2, cg2 = flat_guides(v, albedo=0.25), flat_guides(v, albedo=2.0)
    want = prev.copy()
    want[..., :3] *= 8
    cases.append(("albedo 0.25 -> 2", prev, pg2, v, cg2, p, want))
    # ... and the floor on both sides: 1 / 64 under a floor of 1 / 16
    pg3, cg3 = flat_guides(v, albedo=1 / 64), flat_guides(v, albedo=1 / 64)
    cases.append(("albedo floor", prev, pg3, v, cg3, temporal.params(max_history=64.0, albedo_floor=1 / 16), prev.copy()))
    return cases


# ---- rejection, one tap at a time: every pixel lands half a pixel right and down, so that four taps of weight 1 / 4 count
PIXEL = (1, 2)   # (row, column) of the pixel looked at; its taps in the definition's order:
TAPS = ((1, 2), (1, 3), (2, 2), (2, 3))


def tap_expectation(prev, accepted, albedo_q=0.5, albedo_p=0.5, max_history=64.0):
    """the definition's sums over the `accepted` taps of PIXEL in order, one float32 operation at a time"""
    hs, hn, bs = [f32(0)] * 3, f32(0), f32(0)
    bw = f32(0.25)
    for t in TAPS:
        if t not in accepted:
            continue
        c = prev[t]
        for k in range(3):
            hs[k] = f32(hs[k] + f32(bw * f32(c[k] / f32(albedo_q))))
        hn = f32(hn + f32(bw * c[3]))
        bs = f32(bs + bw)
    if not bs > 0:
        return NONE
    hl = f32(hn / bs)
    return np.array([f32(f32(hs[k] / bs) * f32(albedo_p)) for k in range(3)] + [hl if hl < max_history else f32(max_history)], f32)


def rejection_cases():
    """(name, prev4, prev_guides, view, cur_guides, params, expected record at PIXEL): one of the four taps changed so that the
    named test does or does not reject it"""
    v = flat_view()
    p = temporal.params(max_history=64.0)   # sigma_depth 0.02, normal_min 0.9 as float32
    den, nmin = f32(f32(p["sigma_depth"]) * f32(1.0)), f32(p["normal_min"])
    cg = flat_guides(v, shift_x=0.5, shift_y=0.5)
    cases = []
    for ti, t in enumerate(TAPS):
        rest = [q for q in TAPS if q != t]

        def case(name, rejected, frame=None, guides=None):
            prev, pg = prev_frame(), flat_guides(v)
            if frame:
                frame(prev)
            if guides:
                guides(pg)
            cases.append((f"tap {ti}: {name}", prev, pg, v, cg, p, tap_expectation(prev, rest if rejected else list(TAPS))))

        case("another class", True, guides=lambda g: g["cls"].__setitem__(t, abi.HIT_SPHERE))
        case("class 0", True, guides=lambda g: g["cls"].__setitem__(t, 0))
        case("count 0", True, frame=lambda f: f.__setitem__(t + (3,), 0.0))
        case("count -1", True, frame=lambda f: f.__setitem__(t + (3,), -1.0))
        for k in range(4):
            for bad in (np.nan, np.inf, -np.inf):
                case(f"{bad} in word {k}", True, frame=lambda f, k=k, bad=bad: f.__setitem__(t + (k,), bad))
        case("normal at normal_min", False, guides=lambda g: g["normal"].__setitem__(t, (0, 0, -nmin)))
        case("normal one ulp below", True, guides=lambda g: g["normal"].__setitem__(t, (0, 0, -np.nextafter(nmin, f32(0)))))
        case("plane distance at den", False, guides=lambda g: g["pos"].__setitem__(t + (2,), den))
        case("plane distance at -den", False, guides=lambda g: g["pos"].__setitem__(t + (2,), -den))
        case("plane distance one ulp above", True, guides=lambda g: g["pos"].__setitem__(t + (2,), np.nextafter(den, f32(1))))
        case("NaN normal", True, guides=lambda g: g["normal"].__setitem__(t, (np.nan, 0, -1)))
    # all four rejected: NONE
    prev, pg = prev_frame(), flat_guides(v)
    for t in TAPS:
        pg["cls"][t] = 0
    cases.append(("all four taps rejected", prev, pg, v, cg, p, NONE))
    return cases


def merge_cases():
    """(hist4, guides, cur4, expected): one row of pixels, each a case of MERGE"""
    nan = np.array([0x7FC12345], np.uint32).view(f32)[0]   # a NaN with a payload
    rows = [
        # hst, class, cur, expected
        ((4, 8, 16, 3), 1, (8, 4, 0, 1), (5, 7, 12, 4)),                    # (h * 3 + c * 1) / 4
        ((1, 2, 3, 2), 2, (3, 2, 1, 2), (2, 2, 2, 4)),
        ((4, 8, 16, 3), 0, (8, 4, 0, 1), (8, 4, 0, 1)),                     # class 0
        ((4, 8, 16, 3), 1, (nan, 4, 0, 1), (nan, 4, 0, 1)),                 # a non-finite word: the bits, payload included
        ((4, 8, 16, 3), 1, (8, np.inf, 0, 1), (8, np.inf, 0, 1)),
        ((4, 8, 16, 3), 1, (8, 4, 0, nan), (8, 4, 0, nan)),
        ((4, 8, 16, 3), 1, (8, 4, 0, -1), (8, 4, 0, -1)),                   # !(n >= 0)
        ((0, 0, 0, 0), 1, (8, 4, 0, 1), (8, 4, 0, 1)),                      # no history
        ((4, 8, 16, 3), 3, (0, 0, 0, 0), (4, 8, 16, 3)),                    # nothing accumulated yet: the history alone
        ((4, 8, 16, 3), 3, (-0.0, 0, 0, -0.0), (4, 8, 16, 3)),
    ]
    n = len(rows)
    hst, cur, want = (np.array([r[k] for r in rows], f32).reshape(1, n, 4) for k in (0, 2, 3))
    for a in (cur, want):   # the payload set by its bits: a conversion on the way into the array may not keep it
        a.view(np.uint32)[0, 3, 0] = a.view(np.uint32)[0, 5, 3] = 0x7FC12345
    g = np.zeros((1, n), dtype=abi.GUIDE)
    g["cls"][0] = [r[1] for r in rows]
    return hst, g, cur, want
