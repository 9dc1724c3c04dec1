"""The numpy model of the device's irradiance probes (k_probe_rays, k_sh_project, csrc/rb_probe.hip) and
of the way back in from a baked grid (k_probe_coeffs, k_probe_light, csrc/rb_probe_light.hip; section 19): the same binary32
operations in the same order, so ``rays`` equals ``rb_probe_rays``, ``project`` over the traced colours equals
``rb_bake_probes``, ``coefficients`` equals ``rb_probe_coefficients`` and ``light`` equals ``rb_light_points`` bit for bit.

``records``  abi.PROBE records from (n, 3) positions
``direction``  the direction of an item from its two draws
``rays``     (origins, normalised directions, seeds) of the (probe, sample) items: uniform on the sphere, world axes
``basis``    the nine real spherical harmonics of bands 0-2 of every direction, (m, 9) float32
``project``  abi.SH9[n]: per probe the ordered sums of colour x basis over its samples, and the valid samples
``coefficients``  abi.SH9[n] sums -> abi.SH9[n] irradiance-over-pi coefficients, the weight 1 (a valid probe) or 0
``light``    abi.LIT[m]: the blend of the eight probes of a regular grid round each point, for the point's normal
``grid_params``  the abi.PROBE_GRID whose probes are ``grid``'s positions

Probe visibility (k_depth_project, k_probe_moments, csrc/rb_probe_depth.hip; k_probe_light_vis, csrc/rb_probe_visibility.hip;
section 20), bit for bit as well:

``oct_texel``      the texel ty * 8 + tx of every vector in the 8 x 8 octahedral map
``depth_project``  abi.PROBE_DEPTH[n]: per probe and texel the ordered sums {r, r r, 1, back face} over its samples' hits
``moments``        sums -> (abi.PROBE_DEPTH[n] moments, the back-face share of every probe)
``light_visible``  ``light`` with every corner's weight times the wrapped cosine and the Chebyshev bound of its map
``oct_centres``    the unit directions through the 64 texel centres, for tests and plots

Host-only conveniences in float64, not part of the bit contract:

``radiance_coefficients``  L_j = (4 pi / weight) sum[j], (n, 9, 3)
``irradiance``             E(n) of Ramamoorthi and Hanrahan 2001 from the coefficients, for any normals
``grid``                   the positions of a regular grid of probes inside a box
``blend64``                ``light``'s blend in float64 with the size of its terms: what tests measure ``light`` against
"""
import numpy as np

from . import abi
from .camera import _unit, sincos_turn
from .hemisphere import draws

f32, f64 = np.float32, np.float64
Y0 = f32(0.282094792)
Y1 = f32(0.488602512)
Y2A = f32(1.09254843)
Y20 = f32(0.315391565)
Y22 = f32(0.546274215)
# the cosine lobe's zonal factors A_l of bands 0, 1, 2 (Ramamoorthi and Hanrahan 2001, eq. 8) per coefficient
LOBE = np.array([np.pi] + [2.0 * np.pi / 3.0] * 3 + [np.pi / 4.0] * 5)
# sums -> coefficients (section 19): K_j = 4 A_l, LOBE times 4 pi / pi, so that sum_j coeff_j Y_j(n) is the irradiance over pi
K_BAND = np.array([f32(12.566371)] + [f32(8.37758)] * 3 + [f32(3.1415927)] * 5, dtype=f32)


def records(pos):
    """abi.PROBE[n] from (n, 3) positions"""
    p = np.asarray(pos, f32).reshape(-1, 3)
    r = np.zeros(len(p), dtype=abi.PROBE)
    r["pos"] = p
    return r


def direction(u1, u2):
    """(m, 3) float32: (s, c) = sincos_turn(u1 2 - 1), z = 1 - (u2 + u2), r = sqrt(1 - z z), d = unit((r c, r s, z)) as
    rb_cast_rays normalises a direction.  u2 = 1 gives z = -1 and r = 0: the pole, no NaN."""
    u1, u2 = np.asarray(u1, f32).reshape(-1), np.asarray(u2, f32).reshape(-1)
    with np.errstate(all="ignore"):
        s, c = sincos_turn((u1 * f32(2.0) - f32(1.0)).astype(f32))
        z = (f32(1.0) - (u2 + u2).astype(f32)).astype(f32)
        r = np.sqrt((f32(1.0) - (z * z).astype(f32)).astype(f32), dtype=f32)
        return _unit(np.stack([(r * c).astype(f32), (r * s).astype(f32), z], axis=1))


def rays(pos, first_sample, samples, seeds=None):
    """(origins (n * samples, 3), directions (n * samples, 3), seeds (n * samples,)) of the items (probe, sample), probe-major
    -- item i * samples + k is sample ``first_sample`` + k of probe i --: what rb_probe_rays returns.  The draws are
    ``hemisphere.draws``' (rb_trace_rays' seed rule, exactly two draws), the direction is ``direction``'s, the origin the
    position as given.  An invalid item (a non-finite position) has direction 0 0 0."""
    pos = np.asarray(pos, f32).reshape(-1, 3)
    dr = draws(len(pos), first_sample, samples, seeds)
    i = dr["surfel"]
    d = direction(dr["u1"], dr["u2"])
    org = pos[i].copy()
    valid = np.isfinite(org).all(1) & np.isfinite(d).all(1) & (d != 0).any(1)
    d[~valid] = 0
    return org, d, dr["seed"]


def basis(d):
    """(m, 9) float32 from (m, 3) directions, used as given: Y0 = 0.282094792, Y1..3 = 0.488602512 (y, z, x),
    Y4, Y5, Y7 = 1.09254843 (x y, y z, x z), Y6 = 0.315391565 (3 (z z) - 1), Y8 = 0.546274215 (x x - y y); one binary32
    operation per step."""
    d = np.asarray(d, f32).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    with np.errstate(all="ignore"):
        cols = [np.full(len(d), Y0, f32), Y1 * y, Y1 * z, Y1 * x,
                Y2A * (x * y).astype(f32), Y2A * (y * z).astype(f32),
                Y20 * ((f32(3.0) * (z * z).astype(f32)).astype(f32) - f32(1.0)).astype(f32),
                Y2A * (x * z).astype(f32), Y22 * ((x * x).astype(f32) - (y * y).astype(f32)).astype(f32)]
    return np.stack([c.astype(f32) for c in cols], axis=1)


def project(d, colours, samples):
    """abi.SH9[n] from the items' directions (n * samples, 3), probe-major as ``rays`` returns them, and their colours
    (n * samples, 3), or (n * samples, 4) with the item's weight behind (1 a valid sample, 0 an invalid one; without it an item
    weighs 1 unless its direction is 0 0 0).  sum[j][ch] starts at +0 and takes colour[ch] * Yj of the samples in ascending
    order, one multiply and one add each; weight adds the items' weights."""
    samples = int(samples)
    d = np.asarray(d, f32).reshape(-1, 3)
    col = np.asarray(colours, f32).reshape(len(d), -1)
    if samples < 1 or len(d) % samples or col.shape[1] not in (3, 4):
        raise ValueError("d and colours: (n * samples, 3) and (n * samples, 3 or 4) are needed")
    n = len(d) // samples
    wgt = col[:, 3] if col.shape[1] == 4 else (d != 0).any(1).astype(f32)
    y = basis(d).reshape(n, samples, 9)
    col, wgt = col[:, :3].reshape(n, samples, 3), wgt.reshape(n, samples)
    out = np.zeros(n, dtype=abi.SH9)
    acc, w = np.zeros((n, 9, 3), f32), np.zeros(n, f32)
    with np.errstate(all="ignore"):
        for k in range(samples):
            acc = (acc + (col[:, k, None, :] * y[:, k, :, None]).astype(f32)).astype(f32)
            w = (w + wgt[:, k]).astype(f32)
    out["sum"], out["weight"] = acc, w
    return out


def radiance_coefficients(sh):
    """(n, 9, 3) float64: L_j = (4 pi / weight) sum[j], the Monte-Carlo estimate of the projection of the arriving radiance
    onto Y_j; a probe without a valid sample is all zero.  ``sh``: abi.SH9 records or an (n, 28) array of their floats."""
    a = np.asarray(sh)
    a = a.view(f32) if a.dtype == abi.SH9 else np.asarray(a, f32)
    a = a.reshape(-1, 28).astype(f64)
    w = a[:, 27]
    scale = np.where(w > 0, 4.0 * np.pi / np.where(w > 0, w, 1.0), 0.0)
    return a[:, :27].reshape(-1, 9, 3) * scale[:, None, None]


def irradiance(sh, normals):
    """(n, m, 3) float64: the irradiance of probe i on a surface of unit normal ``normals[m]``, E(n) = pi L0 Y0 + (2 pi / 3)
    sum_{j = 1..3} L_j Y_j(n) + (pi / 4) sum_{j = 4..8} L_j Y_j(n) (Ramamoorthi and Hanrahan 2001).  E / pi is what
    ``bake.irradiance_device`` estimates at the same point and normal."""
    L = radiance_coefficients(sh)
    y = basis(np.asarray(normals, f32).reshape(-1, 3)).astype(f64) * LOBE[None, :]
    return np.einsum("mj,njc->nmc", y, L)


def grid(lo, hi, counts):
    """(nx * ny * nz, 3) float32 positions of a regular grid of probes: along each axis ``counts`` cell centres of the box
    ``lo`` .. ``hi``, x fastest"""
    lo, hi = np.asarray(lo, f64).reshape(3), np.asarray(hi, f64).reshape(3)
    counts = [int(c) for c in counts]
    if len(counts) != 3 or min(counts) < 1:
        raise ValueError("counts: three numbers of at least 1")
    ax = [lo[a] + (np.arange(counts[a]) + 0.5) / counts[a] * (hi[a] - lo[a]) for a in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(f32)


# ---- the way back in: a baked grid lights points
def _sh_floats(sh, what):
    """(n, 28) float32 of abi.SH9 records or of an array of their floats, a copy"""
    a = np.asarray(sh)
    a = a.view(f32) if a.dtype == abi.SH9 else np.asarray(a, f32)
    if a.size % 28:
        raise ValueError(f"{what}: abi.SH9 records or (n, 28) floats are needed")
    return a.reshape(-1, 28).copy()


def coefficients(sh):
    """abi.SH9[n] coefficients of abi.SH9[n] sums (or (n, 28) floats): a probe is valid if its weight is finite and > 0; then
    coeff[j][ch] = (sum[j][ch] * K_j) / weight and the weight word is 1.0; an invalid probe is all-zero bits."""
    a = _sh_floats(sh, "sh")
    w = a[:, 27]
    with np.errstate(all="ignore"):
        valid = (w > 0) & (w < np.inf)
        c = ((a[:, :27].reshape(-1, 9, 3) * K_BAND[None, :, None]).astype(f32) / w[:, None, None]).astype(f32)
    out = np.zeros(len(a), dtype=abi.SH9)
    out["sum"][valid] = c[valid]
    out["weight"][valid] = f32(1.0)
    return out


def grid_params(lo, hi, counts):
    """The abi.PROBE_GRID scalar of ``grid(lo, hi, counts)``: origin = the first cell centre, step = the cell size (a count of
    1: the box size, which nothing reads).  Its probe positions origin + i * step agree with ``grid``'s to rounding."""
    lo, hi = np.asarray(lo, f64).reshape(3), np.asarray(hi, f64).reshape(3)
    counts = [int(c) for c in counts]
    if len(counts) != 3 or min(counts) < 1:
        raise ValueError("counts: three numbers of at least 1")
    g = np.zeros(1, dtype=abi.PROBE_GRID)
    cell = (hi - lo) / np.array(counts, f64)
    g["origin"], g["step"], g["counts"] = lo + 0.5 * cell, cell, counts
    return g[0]


def _cell(grid, pos):
    """per axis the lower probe's index (m, 3) uint32 and the share t (m, 3) float32 of the way to the upper one"""
    g = np.asarray(grid, dtype=abi.PROBE_GRID).reshape(())
    org, step, cnt = g["origin"].astype(f32), g["step"].astype(f32), g["counts"].astype(np.int64)
    with np.errstate(all="ignore"):
        f = ((pos - org[None, :]).astype(f32) / step[None, :]).astype(f32)
        f = np.where(f > 0, f, f32(0.0)).astype(f32)
        top = (cnt - 1).astype(f32)[None, :]
        f = np.where(f < top, f, top).astype(f32)
        i0 = np.minimum(np.floor(f).astype(np.int64), np.maximum(cnt - 2, 0)[None, :])
        t = (f - i0.astype(f32)).astype(f32)
    return i0, t, cnt


def _corners(i0, t, cnt):
    """the eight corners in the definition's order: (record index (m,), geometric weight (m,) float32, exists) each"""
    one = f32(1.0)
    u = (one - t).astype(f32)
    for c in range(8):
        d = (c & 1, (c >> 1) & 1, c >> 2)
        exists = all(cnt[a] >= 2 for a in range(3) if d[a])
        w = [t[:, a] if d[a] else u[:, a] for a in range(3)]
        ii = [i0[:, a] + (d[a] if cnt[a] >= 2 else 0) for a in range(3)]
        yield (ii[2] * cnt[1] + ii[1]) * cnt[0] + ii[0], ((w[0] * w[1]).astype(f32) * w[2]).astype(f32), exists


def _points(pos, normals):
    pos, nrm = np.asarray(pos, f32).reshape(-1, 3), np.asarray(normals, f32).reshape(-1, 3)
    if len(pos) != len(nrm):
        raise ValueError("pos and normals differ in length")
    with np.errstate(all="ignore"):
        len2 = ((nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]).astype(f32) + nrm[:, 2] * nrm[:, 2]).astype(f32)
    valid = np.isfinite(pos).all(1) & np.isfinite(nrm).all(1) & (nrm != 0).any(1) & np.isfinite(len2)
    return pos, nrm, valid


def _blend(grid, coeffs, pos, normals, corner_weight):
    """section 19's stage 2; ``corner_weight(tl, c, idx, pos, unit normals, i0)`` -> (m,) float32 extends a corner's weight
    (section 20), None leaves it"""
    pos, nrm, valid = _points(pos, normals)
    co = _sh_floats(coeffs, "coeffs")
    i0, t, cnt = _cell(grid, pos)
    if len(co) != int(cnt[0] * cnt[1] * cnt[2]):
        raise ValueError("coeffs: nx * ny * nz records are needed")
    m = len(pos)
    n = _unit(nrm)
    y = basis(n)
    E, W = np.zeros((m, 3), f32), np.zeros(m, f32)
    with np.errstate(all="ignore"):
        for c, (idx, wg, exists) in enumerate(_corners(i0, t, cnt)):
            if not exists:
                continue
            rec = co[idx]
            w = (wg * rec[:, 27]).astype(f32)
            if corner_weight is not None:   # (a corner with tl == 0 stays 0 or becomes NaN * 0: skipped either way ...
                w = np.where(w == 0, w, corner_weight(w, c, idx, pos, n, i0)).astype(f32)   # ... so it is left as it is)
            e = np.zeros((m, 3), f32)
            for j in range(9):
                e = (e + (rec[:, 3 * j:3 * j + 3] * y[:, j:j + 1]).astype(f32)).astype(f32)
            take = ~(w == 0)   # (a NaN weight is not 0: it is taken, as on the device)
            E = np.where(take[:, None], (E + (w[:, None] * e).astype(f32)).astype(f32), E)
            W = np.where(take, (W + w).astype(f32), W)
        q = (E / W[:, None]).astype(f32)
        lit = valid & (W > 0)
    out = np.zeros(m, dtype=abi.LIT)
    out["value"][lit] = np.where(q > 0, q, f32(0.0)).astype(f32)[lit]
    out["weight"][lit] = W[lit]
    return out


def light(grid, coeffs, pos, normals):
    """abi.LIT[m] of (m, 3) points and normals from an abi.PROBE_GRID and its coefficient records (``coefficients``' output,
    ``grid``'s order): section 19's stage 2, operation for operation.  ``value`` is the irradiance over pi; ``weight`` the
    blend weight W that was left after invalid probes dropped out (0: nothing lit the point, or the point is invalid)."""
    return _blend(grid, coeffs, pos, normals, None)


def blend64(grid, coeffs, pos, normals, corner_values=None):
    """``light``'s blend in float64 from the same binary32 cell indices and shares: (value (m, 3) before the clamp at 0,
    W (m,), size (m, 3) = sum |w_c coeff Y| / W, the yardstick of a rounding-error bound).  ``corner_values(idx, unit
    normals)`` -> (m, 3) replaces the nine-term dot product of a corner (a reference that evaluates the probes another way)."""
    pos, nrm, valid = _points(pos, normals)
    co = _sh_floats(coeffs, "coeffs").astype(f64)
    i0, t, cnt = _cell(grid, pos)
    m = len(pos)
    n64 = nrm.astype(f64)
    with np.errstate(all="ignore"):
        n64 = n64 / np.sqrt((n64 * n64).sum(1))[:, None]
    x, yy, z = n64[:, 0], n64[:, 1], n64[:, 2]
    y = np.stack([np.full(m, f64(Y0)), f64(Y1) * yy, f64(Y1) * z, f64(Y1) * x, f64(Y2A) * x * yy, f64(Y2A) * yy * z,
                  f64(Y20) * (3.0 * z * z - 1.0), f64(Y2A) * x * z, f64(Y22) * (x * x - yy * yy)], axis=1)
    E, S, W = np.zeros((m, 3)), np.zeros((m, 3)), np.zeros(m)
    t64 = t.astype(f64)
    for c, (idx, _, exists) in enumerate(_corners(i0, t, cnt)):
        if not exists:
            continue
        d = (c & 1, (c >> 1) & 1, c >> 2)
        wg = np.prod([t64[:, a] if d[a] else 1.0 - t64[:, a] for a in range(3)], axis=0)
        rec = co[idx]
        w = wg * rec[:, 27]
        terms = rec[:, :27].reshape(m, 9, 3) * y[:, :, None]
        e = terms.sum(1) if corner_values is None else np.asarray(corner_values(idx, n64), f64)
        take = w != 0
        E += np.where(take[:, None], w[:, None] * e, 0.0)
        S += np.where(take[:, None], np.abs(w)[:, None] * np.abs(terms).sum(1), 0.0)
        W += np.where(take, w, 0.0)
    with np.errstate(all="ignore"):
        return E / W[:, None], W, S / W[:, None]


# ---- probe visibility
def _vec3(v):
    return np.asarray(v, f32).reshape(-1, 3)


def oct_texel(v):
    """(m,) int64 texels ty * 8 + tx of (m, 3) vectors of any length: s = (|x| + |y|) + |z|, p = (x, y) / s, the lower half
    (z < 0; -0 is not) folded over the diagonals, t = min(uint(floor((p 0.5 + 0.5) 8)), 7).  The zero vector and non-finite
    vectors have no texel by the definition; here they get texel 0."""
    v = _vec3(v)
    with np.errstate(all="ignore"):
        a = np.abs(v)
        s = ((a[:, 0] + a[:, 1]).astype(f32) + a[:, 2]).astype(f32)
        px, py = (v[:, 0] / s).astype(f32), (v[:, 1] / s).astype(f32)
        one = f32(1.0)
        fx = ((one - np.abs(py)).astype(f32) * np.where(px >= 0, one, -one).astype(f32)).astype(f32)
        fy = ((one - np.abs(px)).astype(f32) * np.where(py >= 0, one, -one).astype(f32)).astype(f32)
        low = v[:, 2] < 0
        px, py = np.where(low, fx, px).astype(f32), np.where(low, fy, py).astype(f32)

        def axis(p):
            f = np.floor((((p * f32(0.5)).astype(f32) + f32(0.5)).astype(f32) * f32(8.0)).astype(f32))
            return np.minimum(np.nan_to_num(f, nan=0.0, posinf=7.0, neginf=0.0).clip(0, 7).astype(np.int64), 7)
        return axis(py) * 8 + axis(px)


def oct_centres():
    """(64, 3) float32 unit directions through the texel centres, texel T = ty * 8 + tx at row T: the inverse of the octahedral
    map at p = ((tx + 0.5) / 4 - 1, (ty + 0.5) / 4 - 1).  Host float64, not part of the bit contract; ``oct_texel`` of row T
    is T."""
    t = (np.arange(8, dtype=f64) + 0.5) / 4.0 - 1.0
    py, px = np.meshgrid(t, t, indexing="ij")
    z = 1.0 - np.abs(px) - np.abs(py)
    low = z < 0
    x = np.where(low, (1.0 - np.abs(py)) * np.where(px >= 0, 1.0, -1.0), px)
    y = np.where(low, (1.0 - np.abs(px)) * np.where(py >= 0, 1.0, -1.0), py)
    d = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)
    return (d / np.sqrt((d * d).sum(1))[:, None]).astype(f32)


def depth_project(dirs, hits, samples, max_distance):
    """abi.PROBE_DEPTH[n] from the items' directions as their records store them ((n * samples, 3), probe-major as ``rays``
    and rb_probe_rays return them) and their abi.HIT records (rb_cast_rays of those records): from all-zero bits in ascending
    sample order, a sample with a zero direction or an invalid hit skipped, texel[oct_texel(d)] += {r, r r, 1, back} with
    r = min(t, max_distance) and back = 1 where a triangle's or a sphere's normal looks along the ray, (n.x d.x + n.y d.y) +
    n.z d.z > 0."""
    samples = int(samples)
    d = _vec3(dirs)
    hits = np.asarray(hits, dtype=abi.HIT).reshape(-1)
    if samples < 1 or len(d) % samples or len(hits) != len(d):
        raise ValueError("dirs and hits: (n * samples, 3) and abi.HIT[n * samples] are needed")
    n = len(d) // samples
    md = f32(max_distance)
    with np.errstate(all="ignore"):
        T = oct_texel(d)
        r = np.where(hits["t"] < md, hits["t"], md).astype(f32)
        r2 = (r * r).astype(f32)
        nr = hits["normal"].astype(f32)
        dt = ((nr[:, 0] * d[:, 0] + nr[:, 1] * d[:, 1]).astype(f32) + nr[:, 2] * d[:, 2]).astype(f32)
    surface = (hits["kind"] == abi.HIT_TRIANGLE) | (hits["kind"] == abi.HIT_SPHERE)
    back = np.where(surface & (dt > 0), f32(1.0), f32(0.0)).astype(f32)
    take = (d != 0).any(1) & (hits["kind"] != abi.HIT_INVALID)
    acc = np.zeros((n, 64, 4), f32)
    rows = np.arange(n)
    T, take = T.reshape(n, samples), take.reshape(n, samples)
    terms = np.stack([r, r2, np.ones_like(r), back], axis=1).reshape(n, samples, 4)
    with np.errstate(all="ignore"):   # (distances near 1e19 and beyond: r r and the sums overflow to inf, as on the device)
        for k in range(samples):   # one sample of every probe at a time: a texel takes its samples in ascending order
            i = rows[take[:, k]]
            acc[i, T[i, k]] = (acc[i, T[i, k]] + terms[i, k]).astype(f32)
    out = np.zeros(n, dtype=abi.PROBE_DEPTH)
    out["texel"] = acc
    return out


def _depth_floats(maps, what):
    a = np.asarray(maps)
    a = a.view(f32) if a.dtype == abi.PROBE_DEPTH else np.asarray(a, f32)
    if a.size % 256:
        raise ValueError(f"{what}: abi.PROBE_DEPTH records or (n, 256) floats are needed")
    return a.reshape(-1, 64, 4).copy()


def moments(sums):
    """(abi.PROBE_DEPTH[n] moments, (n,) float32 back-face shares) of abi.PROBE_DEPTH[n] sums: a texel whose count is finite
    and > 0 becomes {sum_r / count, sum_r2 / count, 1, back / count}, any other all-zero bits; the share is B / C, 0 where
    C == 0, B and C the sums of ``back`` and ``count`` over the texels in ascending order from +0."""
    a = _depth_floats(sums, "sums")
    cnt = a[:, :, 2]
    with np.errstate(all="ignore"):
        valid = (cnt > 0) & (cnt < np.inf)
        q = (a / cnt[:, :, None]).astype(f32)
        q[:, :, 2] = f32(1.0)
        B, C = np.zeros(len(a), f32), np.zeros(len(a), f32)
        for t in range(64):
            B, C = (B + a[:, t, 3]).astype(f32), (C + a[:, t, 2]).astype(f32)
        share = np.where(C == 0, f32(0.0), (B / C).astype(f32)).astype(f32)
    out = np.zeros(len(a), dtype=abi.PROBE_DEPTH)
    out["texel"] = np.where(valid[:, :, None], q, f32(0.0))
    return out, share


def visibility_params(normal_bias=0.0, min_visibility=0.0, wrap=True, depth=True):
    """the abi.LIGHT_VISIBILITY scalar of these settings"""
    p = np.zeros(1, dtype=abi.LIGHT_VISIBILITY)
    p["normal_bias"], p["min_visibility"] = normal_bias, min_visibility
    p["flags"] = (0 if wrap else abi.VIS_NO_WRAP) | (0 if depth else abi.VIS_NO_DEPTH)
    return p[0]


def _dot3(a, b):
    return ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]).astype(f32) + a[:, 2] * b[:, 2]).astype(f32)


def light_visible(grid, coeffs, moment_maps, pos, normals, params):
    """abi.LIT[m] as ``light``, every corner's weight tl extended to (tl * wb) * vis (section 20): wb = h h + 0.2 with
    h = (cos + 1) 0.5 of the angle between the unit normal and the direction to the probe (1 at the probe itself; 1 under
    VIS_NO_WRAP), vis = max(Chebyshev bound cubed, min_visibility) of the distance r from the probe to the point moved
    ``normal_bias`` along its normal against the moments of texel oct_texel(point - probe) -- 1 where r is 0, the texel has no
    sample or r is not beyond the mean, and under VIS_NO_DEPTH, where ``moment_maps`` may be None.  ``params``: an
    abi.LIGHT_VISIBILITY scalar (``visibility_params``)."""
    g = np.asarray(grid, dtype=abi.PROBE_GRID).reshape(())
    prm = np.asarray(params, dtype=abi.LIGHT_VISIBILITY).reshape(())
    org, step = g["origin"].astype(f32), g["step"].astype(f32)
    flags, bias, floor = int(prm["flags"]), f32(prm["normal_bias"]), f32(prm["min_visibility"])
    depth = not flags & abi.VIS_NO_DEPTH
    mm = _depth_floats(moment_maps, "moments") if depth else None
    one = f32(1.0)

    def corner_weight(tl, c, idx, p, n, i0):
        d = (c & 1, (c >> 1) & 1, c >> 2)
        P = np.stack([(org[a] + ((i0[:, a] + d[a]).astype(f32) * step[a]).astype(f32)).astype(f32) for a in range(3)], axis=1)
        wb = np.ones(len(p), f32)
        if not flags & abi.VIS_NO_WRAP:
            q = (P - p).astype(f32)
            l = np.sqrt(_dot3(q, q), dtype=f32)
            cw = np.where(l > 0, (_dot3(q, n) / l).astype(f32), one).astype(f32)
            h = ((cw + one).astype(f32) * f32(0.5)).astype(f32)
            wb = ((h * h).astype(f32) + f32(0.2)).astype(f32)
        vis = np.ones(len(p), f32)
        if depth:
            v = ((p + (n * bias).astype(f32)).astype(f32) - P).astype(f32)
            r = np.sqrt(_dot3(v, v), dtype=f32)
            tex = mm[idx, oct_texel(v)]
            mean, mean2 = tex[:, 0], tex[:, 1]
            var = np.abs((mean2 - (mean * mean).astype(f32)).astype(f32))
            dl = (r - mean).astype(f32)
            den = (var + (dl * dl).astype(f32)).astype(f32)
            ch = np.where(den > 0, (var / den).astype(f32), one).astype(f32)
            open_ = (r == 0) | (tex[:, 2] == 0) | ~(r > mean)
            vis = np.where(open_, one, ((ch * ch).astype(f32) * ch).astype(f32)).astype(f32)
        vis = np.where(vis > floor, vis, floor).astype(f32)
        return ((tl * wb).astype(f32) * vis).astype(f32)

    if mm is not None and len(mm) != int(np.prod(g["counts"].astype(np.int64))):
        raise ValueError("moments: nx * ny * nz maps are needed")
    return _blend(grid, coeffs, pos, normals, corner_weight)
