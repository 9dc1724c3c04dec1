"""DESIGN.md sections 19.1 (stage 1 and stage 2) and 20.1 (the texel, the moments, the visible blend) once more, for one probe or
one point at a time: plain Python control flow on np.float32 scalars, one operation per line, written from the DESIGN text.  It
shares nothing with renderbaby_amd/probes.py and evaluates no branch the definition does not take, which is what makes it the
judge between the vectorised model and the device (tests/test_probe_edges_model.py, tests/test_gpu_probe_edges.py).

``coefficients_one``  28 floats of sums -> 28 floats of coefficients
``moments_one``       (64, 4) sums of a map -> ((64, 4) moments, the back-face share)
``texel``             the texel of a vector, and ``texel_axes`` its (tx, ty, lower half)
``light_one``         one point from a grid's records: section 19.1's stage 2, or with ``vis`` section 20.1's blend
``coefficients``, ``moments``, ``light``: the same over arrays, for the tests

Callers wrap the calls in ``np.errstate(all="ignore")``: overflow, 0 / 0 and inf - inf are what the cases are about.
"""
import numpy as np

f32 = np.float32
ZERO, ONE, HALF, INF = f32(0.0), f32(1.0), f32(0.5), f32(np.inf)
K = [f32(12.566371)] + [f32(8.37758)] * 3 + [f32(3.1415927)] * 5
C0, C1, C2A, C20, C22 = f32(0.282094792), f32(0.488602512), f32(1.09254843), f32(0.315391565), f32(0.546274215)
VIS_NO_WRAP, VIS_NO_DEPTH = 1, 2


def finite(x):
    return x == x and x != INF and x != -INF


# ---- section 19.1, stage 1
def coefficients_one(rec):
    w = f32(rec[27])
    out = [ZERO] * 28
    if not (w > ZERO and w < INF):   # "finite and greater than 0"; a NaN is neither
        return out
    for j in range(9):
        for ch in range(3):
            p = f32(f32(rec[3 * j + ch]) * K[j])
            out[3 * j + ch] = f32(p / w)
    out[27] = ONE
    return out


# ---- section 20.1, the moments
def moments_one(tex):
    out = [[ZERO] * 4 for _ in range(64)]
    for t in range(64):
        sum_r, sum_r2, count, back = (f32(x) for x in tex[t])
        if count > ZERO and finite(count):
            out[t] = [f32(sum_r / count), f32(sum_r2 / count), ONE, f32(back / count)]
    B, C = ZERO, ZERO
    for t in range(64):
        B = f32(B + f32(tex[t][3]))
        C = f32(C + f32(tex[t][2]))
    share = ZERO if C == ZERO else f32(B / C)
    return out, share


# ---- section 20.1, the texel
def _texel_axis(p):
    f = f32(f32(f32(p * HALF) + HALF) * f32(8.0))
    if not f >= ZERO:      # "a texel index is clamped whatever it is computed from": below 0 and NaN give 0 ...
        return 0
    if f >= f32(7.0):      # ... and 7 and above, +inf included, give 7
        return 7
    return int(np.floor(f))


def texel_axes(v):
    x, y, z = (f32(c) for c in v)
    s = f32(f32(abs(x) + abs(y)) + abs(z))
    px = f32(x / s)
    py = f32(y / s)
    low = bool(z < ZERO)
    if low:
        sx = ONE if px >= ZERO else -ONE
        sy = ONE if py >= ZERO else -ONE
        fx = f32(f32(ONE - abs(py)) * sx)
        fy = f32(f32(ONE - abs(px)) * sy)
        px, py = fx, fy
    return _texel_axis(px), _texel_axis(py), low


def texel(v):
    tx, ty, _ = texel_axes(v)
    return ty * 8 + tx


# ---- section 18.1's basis
def basis_one(x, y, z):
    return [C0, f32(C1 * y), f32(C1 * z), f32(C1 * x), f32(C2A * f32(x * y)), f32(C2A * f32(y * z)),
            f32(C20 * f32(f32(f32(3.0) * f32(z * z)) - ONE)), f32(C2A * f32(x * z)), f32(C22 * f32(f32(x * x) - f32(y * y)))]


def dot3(a, b):
    return f32(f32(f32(a[0] * b[0]) + f32(a[1] * b[1])) + f32(a[2] * b[2]))


# ---- section 19.1, stage 2, and section 20.1's blend
def light_one(origin, step, counts, coeffs, pos, nrm, vis=None):
    """``coeffs``: (n, 28) float32; ``vis``: None or dict(moments=(n, 64, 4) float32 or None, normal_bias, min_visibility,
    flags)"""
    nothing = [ZERO] * 4
    pos = [f32(c) for c in pos]
    nrm = [f32(c) for c in nrm]
    if not all(finite(c) for c in pos) or not all(finite(c) for c in nrm):
        return nothing
    if nrm[0] == ZERO and nrm[1] == ZERO and nrm[2] == ZERO:
        return nothing
    len2 = dot3(nrm, nrm)
    if not finite(len2):
        return nothing
    ln = f32(np.sqrt(len2))
    n = [f32(c / ln) for c in nrm]
    Y = basis_one(*n)
    i0, t = [0] * 3, [ZERO] * 3
    for a in range(3):
        f = f32(f32(pos[a] - f32(origin[a])) / f32(step[a]))
        f = f if f > ZERO else ZERO
        top = f32(int(counts[a]) - 1)
        f = f if f < top else top
        i0[a] = min(int(np.floor(f)), int(counts[a]) - 2 if int(counts[a]) >= 2 else 0)
        t[a] = f32(f - f32(i0[a]))
    E, W = [ZERO] * 3, ZERO
    for c in range(8):
        d = (c & 1, (c >> 1) & 1, c >> 2)
        if any(d[a] and int(counts[a]) == 1 for a in range(3)):
            continue   # the corner does not exist
        wa = [t[a] if d[a] else f32(ONE - t[a]) for a in range(3)]
        ii = [i0[a] + d[a] for a in range(3)]
        rec = coeffs[(ii[2] * int(counts[1]) + ii[1]) * int(counts[0]) + ii[0]]
        w = f32(f32(f32(wa[0] * wa[1]) * wa[2]) * f32(rec[27]))
        if w == ZERO:
            continue   # skipped entirely
        if vis is not None:
            flags = int(vis["flags"])
            P = [f32(f32(origin[a]) + f32(f32(ii[a]) * f32(step[a]))) for a in range(3)]
            wb = ONE
            if not flags & VIS_NO_WRAP:
                q = [f32(P[a] - pos[a]) for a in range(3)]
                l = f32(np.sqrt(dot3(q, q)))
                cw = f32(dot3(q, n) / l) if l > ZERO else ONE
                h = f32(f32(cw + ONE) * HALF)
                wb = f32(f32(h * h) + f32(0.2))
            v1 = ONE
            if not flags & VIS_NO_DEPTH:
                bias = f32(vis["normal_bias"])
                b = [f32(pos[a] + f32(n[a] * bias)) for a in range(3)]
                v = [f32(b[a] - P[a]) for a in range(3)]
                r = f32(np.sqrt(dot3(v, v)))
                if not r == ZERO:
                    mean, mean2, valid, _ = (f32(x) for x in vis["moments"][(ii[2] * int(counts[1]) + ii[1]) * int(counts[0]) + ii[0]][texel(v)])
                    if not (valid == ZERO or not r > mean):
                        var = abs(f32(mean2 - f32(mean * mean)))
                        dl = f32(r - mean)
                        den = f32(var + f32(dl * dl))
                        ch = f32(var / den) if den > ZERO else ONE
                        v1 = f32(f32(ch * ch) * ch)
            floor = f32(vis["min_visibility"])
            v1 = v1 if v1 > floor else floor
            w = f32(f32(w * wb) * v1)
            if w == ZERO:
                continue
        for ch in range(3):
            e = ZERO
            for j in range(9):
                e = f32(e + f32(f32(rec[3 * j + ch]) * Y[j]))
            E[ch] = f32(E[ch] + f32(w * e))
        W = f32(W + w)
    if not W > ZERO:
        return nothing
    out = []
    for ch in range(3):
        q = f32(E[ch] / W)
        out.append(q if q > ZERO else ZERO)
    return out + [W]


# ---- over arrays
def coefficients(sh28):
    a = np.asarray(sh28, f32).reshape(-1, 28)
    with np.errstate(all="ignore"):
        return np.array([coefficients_one(r) for r in a], f32).reshape(-1, 28)


def moments(maps):
    a = np.asarray(maps, f32).reshape(-1, 64, 4)
    with np.errstate(all="ignore"):
        got = [moments_one(m) for m in a]
    return np.array([g[0] for g in got], f32).reshape(-1, 256), np.array([g[1] for g in got], f32)


def light(grid, coeffs28, pos, nrm, vis=None):
    """(m, 4) float32; ``grid``: an abi.PROBE_GRID scalar; ``vis``: None or (moments (n, 256) or None, abi.LIGHT_VISIBILITY scalar)"""
    co = np.asarray(coeffs28, f32).reshape(-1, 28)
    pos, nrm = np.asarray(pos, f32).reshape(-1, 3), np.asarray(nrm, f32).reshape(-1, 3)
    v = None
    if vis is not None:
        maps, prm = vis
        v = dict(moments=None if maps is None else np.asarray(maps, f32).reshape(-1, 64, 4), normal_bias=prm["normal_bias"],
                 min_visibility=prm["min_visibility"], flags=prm["flags"])
    with np.errstate(all="ignore"):
        return np.array([light_one(grid["origin"], grid["step"], grid["counts"], co, p, n, v) for p, n in zip(pos, nrm)], f32).reshape(-1, 4)
