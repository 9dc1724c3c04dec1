"""The numpy model of the device's irradiance probes (k_probe_rays, k_sh_project, csrc/rb_probe.hip): the
same binary32 operations in the same order, so ``rays`` equals ``rb_probe_rays`` and ``project`` over the traced colours equals
``rb_bake_probes`` bit for bit.

``records``  abi.PROBE records from (n, 3) positions
``direction``  the direction of an item from its two draws
``rays``     (origins, normalised directions, seeds) of the (probe, sample) items: uniform on the sphere, world axes
``basis``    the nine real spherical harmonics of bands 0-2 of every direction, (m, 9) float32
``project``  abi.SH9[n]: per probe the ordered sums of colour x basis over its samples, and the valid samples

Host-only conveniences in float64, not part of the bit contract:

``radiance_coefficients``  L_j = (4 pi / weight) sum[j], (n, 9, 3)
``irradiance``             E(n) of Ramamoorthi and Hanrahan 2001 from the coefficients, for any normals
``grid``                   the positions of a regular grid of probes inside a box
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
