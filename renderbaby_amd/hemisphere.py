"""The numpy model of the device's hemisphere-ray generator (k_hemi_rays, csrc/rb_hemisphere.hip):
the same binary32 operations in the same order, so ``rays`` equals ``rb_hemisphere_rays`` bit for bit.

``surfels``  abi.SURFEL records from (m, 3) points and normals
``frame``    (nrm, t1, t2) of every normal: the device's normalisation and the branch-free tangent frame of Duff et al. 2017
``draws``    what the generator draws for every (surfel, sample) item
``local``    the direction of an item from its frame and its two draws, before the last normalisation
``rays``     (origins, normalised directions, seeds) of the items: the records ``rb_hemisphere_rays`` returns
"""
import numpy as np

from . import abi
from .camera import _unit, pcg, random_float, sincos_turn

f32, u32, u64 = np.float32, np.uint32, np.uint64


def surfels(points, normals):
    """abi.SURFEL[m] from (m, 3) points and normals (any length: the device normalises)"""
    p = np.asarray(points, f32).reshape(-1, 3)
    n = np.asarray(normals, f32).reshape(-1, 3)
    if len(p) != len(n):
        raise ValueError("points and normals differ in length")
    s = np.zeros(len(p), dtype=abi.SURFEL)
    s["pos"], s["normal"] = p, n
    return s


def frame(normals):
    """(nrm, t1, t2), each (m, 3) float32: nrm = the normal normalised as rb_cast_rays normalises a direction;
    sg = copysign(1, nrm.z), a = -1 / (sg + nrm.z), b = (nrm.x nrm.y) a,
    t1 = (1 + (sg (nrm.x nrm.x)) a, sg b, (-sg) nrm.x), t2 = (b, sg + (nrm.y nrm.y) a, -nrm.y)."""
    with np.errstate(all="ignore"):
        nrm = _unit(np.asarray(normals, f32).reshape(-1, 3))
        x, y, z = nrm[:, 0], nrm[:, 1], nrm[:, 2]
        sg = np.copysign(f32(1.0), z).astype(f32)
        a = (f32(-1.0) / (sg + z).astype(f32)).astype(f32)
        b = ((x * y).astype(f32) * a).astype(f32)
        t1 = np.stack([(f32(1.0) + ((sg * (x * x).astype(f32)).astype(f32) * a).astype(f32)).astype(f32),
                       (sg * b).astype(f32), ((-sg) * x).astype(f32)], axis=1)
        t2 = np.stack([b, (sg + ((y * y).astype(f32) * a).astype(f32)).astype(f32), -y], axis=1)
    return nrm, t1.astype(f32), t2.astype(f32)


def draws(m, first_sample, samples, seeds=None):
    """What the generator draws for the items (surfel, sample) of ``m`` surfels, surfel-major: dict of ``seed`` (the state
    after the two draws: what trace_ray starts with), ``u1``, ``u2`` and ``surfel`` (the item's surfel).  ``seeds``: the
    surfels' ids, by default their indices -- rb_trace_rays' rule."""
    sid = np.arange(m, dtype=u64) if seeds is None else np.asarray(seeds, u32).reshape(-1).astype(u64)
    if len(sid) != m:
        raise ValueError("seeds: one id per surfel is needed")
    surfel = np.repeat(np.arange(m, dtype=np.int64), samples)
    k = np.tile(np.arange(samples, dtype=u64), m)
    hs = pcg((u64(first_sample) + k) & u64(0xFFFFFFFF))
    seed = pcg((sid[surfel] + hs.astype(u64)) & u64(0xFFFFFFFF))
    seed, u1 = random_float(seed)
    seed, u2 = random_float(seed)
    return dict(seed=seed, u1=u1, u2=u2, surfel=surfel)


def local(nrm, t1, t2, u1, u2):
    """d = ((r c) t1 + (r s) t2) + z nrm per item, (s, c) = sincos_turn(u1 2 - 1), r = sqrt(u2), z = sqrt(1 - u2); not yet
    normalised.  All arguments per item."""
    u1, u2 = np.asarray(u1, f32), np.asarray(u2, f32)
    with np.errstate(all="ignore"):
        s, c = sincos_turn((u1 * f32(2.0) - f32(1.0)).astype(f32))
        r = np.sqrt(u2, dtype=f32)
        z = np.sqrt((f32(1.0) - u2).astype(f32), dtype=f32)
        rc, rs = (r * c).astype(f32), (r * s).astype(f32)
        return (((rc[:, None] * t1).astype(f32) + (rs[:, None] * t2).astype(f32)).astype(f32) + (z[:, None] * nrm).astype(f32)).astype(f32)


def rays(surf, first_sample, samples, seeds=None, offset=1e-3):
    """(origins (n, 3), directions (n, 3), seeds (n,)) of the items (surfel, sample), surfel-major -- item i * samples + k is
    sample ``first_sample`` + k of ``surf[i]`` --: what rb_hemisphere_rays returns.  The directions are normalised; an invalid
    item (section 16.1) has its surfel's position as given and direction 0 0 0."""
    surf = np.asarray(surf, dtype=abi.SURFEL).reshape(-1)
    pos = surf["pos"].astype(f32)
    dr = draws(len(surf), first_sample, samples, seeds)
    i = dr["surfel"]
    nrm, t1, t2 = frame(surf["normal"])
    with np.errstate(all="ignore"):
        ok = np.isfinite(pos).all(1) & np.isfinite(nrm).all(1) & (nrm != 0).any(1)
        d = _unit(local(nrm[i], t1[i], t2[i], dr["u1"], dr["u2"]))
        px, py, pz = pos[:, 0], pos[:, 1], pos[:, 2]
        reach = np.sqrt((((px * px).astype(f32) + (py * py).astype(f32)).astype(f32) + (pz * pz).astype(f32)).astype(f32), dtype=f32)
        step = (f32(offset) * np.where(reach > f32(1.0), reach, f32(1.0)).astype(f32)).astype(f32)
        org = (pos + (step[:, None] * nrm).astype(f32)).astype(f32)[i]
    valid = ok[i] & np.isfinite(org).all(1) & np.isfinite(d).all(1) & (d != 0).any(1)
    org[~valid] = pos[i][~valid]
    d[~valid] = 0
    return org, d, dr["seed"]
