"""The numpy model of the device's camera-ray generator (k_cam_rays, csrc/rb_camera.hip): the same
binary32 operations in the same order, so ``rays`` equals ``rb_camera_rays`` bit for bit.

``make``         an abi.CAMERA_EX record from a position, a viewing direction and the parameters of its kind
``rays``         (origins, normalised directions, seeds) of (pixel, sample) items: the records ``rb_camera_rays`` returns
``sincos_turn``  sin and cos of pi * s, the fixed polynomial routine the equirect camera uses
"""
import numpy as np

from . import abi

f32, u32, u64 = np.float32, np.uint32, np.uint64
KINDS = {"perspective": abi.CAM_PERSPECTIVE, "ortho": abi.CAM_ORTHO, "equirect": abi.CAM_EQUIRECT}
PI = f32(np.pi)
SIN_COEFFS = tuple(f32(c) for c in (1.0 / 362880.0, -1.0 / 5040.0, 1.0 / 120.0, -1.0 / 6.0, 1.0))
COS_COEFFS = tuple(f32(c) for c in (1.0 / 40320.0, -1.0 / 720.0, 1.0 / 24.0, -1.0 / 2.0, 1.0))


def _unit(v):
    v = np.asarray(v, f32)
    with np.errstate(all="ignore"):
        return (v / np.sqrt((v[..., 0:1] * v[..., 0:1] + v[..., 1:2] * v[..., 1:2]) + v[..., 2:3] * v[..., 2:3], dtype=f32)).astype(f32)


def make(kind, width, height, pos, dir=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), fov_deg=60.0, ortho_width=2.0, aperture=0.0,
         focus_distance=1.0, jitter=True):
    """An abi.CAMERA_EX scalar.  ``kind``: "perspective" (vertical field of view ``fov_deg``; ``aperture`` is the lens
    DIAMETER, 0 = pinhole; ``focus_distance`` is that of the focal plane along ``dir``), "ortho" (a window ``ortho_width``
    wide, its height by the image's aspect) or "equirect".  The basis is orthonormal: forward = unit ``dir``, right =
    unit(forward x ``up``), up = right x forward -- bake.camera_rays' basis."""
    if kind not in KINDS:
        raise ValueError(f"unknown camera {kind!r}: one of {', '.join(KINDS)}")
    w, h = int(width), int(height)
    if w < 1 or h < 1:
        raise ValueError("width and height must be at least 1")
    fwd = _unit(np.asarray(dir, f32).reshape(3))
    right = np.cross(fwd, np.asarray(up, f32).reshape(3)).astype(f32)
    if not np.any(right):
        raise ValueError("dir and up are parallel")
    right = _unit(right)
    cam = np.zeros((), dtype=abi.CAMERA_EX)
    cam["kind"], cam["width"], cam["height"] = KINDS[kind], w, h
    cam["flags"] = 0 if jitter else abi.CAM_NO_JITTER
    cam["pos"], cam["right"], cam["up"], cam["forward"] = np.asarray(pos, f32).reshape(3), right, np.cross(right, fwd).astype(f32), fwd
    cam["tan_half_fov"] = f32(np.tan(np.radians(fov_deg) / 2.0))
    cam["half_width"] = f32(ortho_width) / f32(2.0)
    cam["half_height"] = cam["half_width"] * f32(h) / f32(w)
    cam["lens_radius"] = f32(aperture) / f32(2.0)
    cam["focus_distance"] = f32(focus_distance)
    return cam


def pcg(v):
    """shader.wgsl:417-421 on uint32 arrays"""
    v = np.asarray(v, u64)
    state = (v * u64(747796405) + u64(2891336453)) & u64(0xFFFFFFFF)
    word = (((state >> ((state >> u64(28)) + u64(4))) ^ state) * u64(277803737)) & u64(0xFFFFFFFF)
    return (((word >> u64(22)) ^ word) & u64(0xFFFFFFFF)).astype(u32)


def random_float(seed):
    """shader.wgsl:423-426: (the advanced seed, (float)seed / 2^32)"""
    seed = pcg(seed)
    return seed, (seed.astype(f32) / f32(4294967296.0)).astype(f32)


def sincos_turn(s):
    """(sin, cos) of pi * s for float32 s in [-1, 1]: the nearest quarter turn q = rint(2 s), r = s - q / 2 (exact),
    x = r * (float)pi, the Taylor polynomials to x^9 and x^8 in Horner form (one multiply, then one add per step), the
    result by the quadrant q mod 4."""
    s = np.asarray(s, f32)
    q = np.rint(f32(2.0) * s).astype(f32)
    r = (s - f32(0.5) * q).astype(f32)
    x = (r * PI).astype(f32)
    x2 = (x * x).astype(f32)
    ps, pc = SIN_COEFFS[0], COS_COEFFS[0]
    for cs, cc in zip(SIN_COEFFS[1:], COS_COEFFS[1:]):
        ps = ((ps * x2).astype(f32) + cs).astype(f32)
        pc = ((pc * x2).astype(f32) + cc).astype(f32)
    sn = (x * ps).astype(f32)
    quad = q.astype(np.int32) & 3
    return (np.select([quad == 0, quad == 1, quad == 2], [sn, pc, -sn], -pc).astype(f32),
            np.select([quad == 0, quad == 1, quad == 2], [pc, -sn, -pc], sn).astype(f32))


def _scaled(a, v):
    """(n,) float32 times a 3-vector -> (n, 3), one multiply per component"""
    return (a[:, None] * v[None, :]).astype(f32)


def draws(cam, pixels, first_sample, samples):
    """What the generator draws for every (pixel, sample) item, pixel-major: dict of ``seed`` (the state after the draws),
    ``jx``, ``jy`` (the jitter offsets as drawn, before RB_CAM_NO_JITTER replaces them), ``lx``, ``ly`` (the accepted lens
    point; zeros without a lens) and ``tries`` (lens candidates drawn)."""
    cam = np.asarray(cam, dtype=abi.CAMERA_EX).reshape(())
    p = np.repeat(np.asarray(pixels, u64).reshape(-1), samples)
    k = np.tile(np.arange(samples, dtype=u64), len(p) // max(samples, 1))
    hs = pcg((u64(first_sample) + k) & u64(0xFFFFFFFF))
    seed = pcg((p + hs.astype(u64)) & u64(0xFFFFFFFF))
    seed, jx = random_float(seed)
    seed, jy = random_float(seed)
    jx, jy = (jx - f32(0.5)).astype(f32), (jy - f32(0.5)).astype(f32)
    lx, ly, tries = np.zeros(len(p), f32), np.zeros(len(p), f32), np.zeros(len(p), np.int32)
    if int(cam["kind"]) == abi.CAM_PERSPECTIVE and f32(cam["lens_radius"]) != 0:
        todo = np.ones(len(p), bool)
        while todo.any():
            s1, a = random_float(seed[todo])
            s2, b = random_float(s1)
            a, b = (a * f32(2.0) - f32(1.0)).astype(f32), (b * f32(2.0) - f32(1.0)).astype(f32)
            seed[todo], lx[todo], ly[todo] = s2, a, b
            tries[todo] += 1
            inside = ((a * a).astype(f32) + (b * b).astype(f32)).astype(f32) < f32(1.0)
            todo[np.nonzero(todo)[0][inside]] = False
    return dict(seed=seed, jx=jx, jy=jy, lx=lx, ly=ly, tries=tries, pixel=p.astype(u32))


def rays(cam, pixels, first_sample, samples):
    """(origins (n, 3), directions (n, 3), seeds (n,)) of the items (pixel, sample), pixel-major -- item i * samples + k is
    sample ``first_sample`` + k of ``pixels[i]`` --: what rb_camera_rays returns.  The directions are normalised; an invalid
    ray (rb_cast_rays' rule) has direction 0 0 0."""
    cam = np.asarray(cam, dtype=abi.CAMERA_EX).reshape(())
    w, h, kind = int(cam["width"]), int(cam["height"]), int(cam["kind"])
    dr = draws(cam, pixels, first_sample, samples)
    p, jx, jy = dr["pixel"], dr["jx"], dr["jy"]
    if int(cam["flags"]) & abi.CAM_NO_JITTER:
        jx, jy = np.zeros_like(jx), np.zeros_like(jy)
    row, col = p // u32(w), p % u32(w)
    pos, right, up, fwd = (cam[n].astype(f32) for n in ("pos", "right", "up", "forward"))
    with np.errstate(all="ignore"):
        sx = ((((col.astype(f32) + f32(0.5)) + jx) / f32(w)) * f32(2.0) - f32(1.0)).astype(f32)
        sy = (f32(1.0) - (((row.astype(f32) + f32(0.5)) + jy) / f32(h)) * f32(2.0)).astype(f32)
        org = np.broadcast_to(pos, (len(p), 3)).astype(f32)
        if kind == abi.CAM_PERSPECTIVE:
            th = f32(cam["tan_half_fov"])
            a = th * (f32(w) / f32(h))
            d = ((_scaled(sx * a, right) + _scaled(sy * th, up)).astype(f32) + fwd).astype(f32)
            radius = f32(cam["lens_radius"])
            if radius != 0:
                org = ((pos + _scaled(radius * dr["lx"], right)).astype(f32) + _scaled(radius * dr["ly"], up)).astype(f32)
                d = ((pos + (f32(cam["focus_distance"]) * d).astype(f32)).astype(f32) - org).astype(f32)
        elif kind == abi.CAM_ORTHO:
            org = ((pos + _scaled(sx * f32(cam["half_width"]), right)).astype(f32) + _scaled(sy * f32(cam["half_height"]), up)).astype(f32)
            d = np.broadcast_to(fwd, (len(p), 3)).astype(f32)
        elif kind == abi.CAM_EQUIRECT:
            sl, cl = sincos_turn(sx)
            sa, ca = sincos_turn((f32(0.5) * sy).astype(f32))
            d = ((_scaled((ca * sl).astype(f32), right) + _scaled(sa, up)).astype(f32) + _scaled((ca * cl).astype(f32), fwd)).astype(f32)
        else:
            raise ValueError(f"unknown camera kind {kind}")
        d = _unit(d)
    valid = np.isfinite(org).all(1) & np.isfinite(d).all(1) & (d != 0).any(1)
    d[~valid] = 0
    return org, d, dr["seed"]
