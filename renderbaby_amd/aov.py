"""First-hit buffers as images: pure numpy over the records of ``Engine.render_hits`` / ``Engine.cast_rays``
(abi.HIT, abi.SURFACE).  No device, no library.

The records are already in the orientation of the delivered RGBA8 frame (row-major, top row first, x mirrored), so every
function here maps record [row, column] to pixel [row, column] and nothing is flipped.  Pixels whose ray hit nothing
(HIT_NONE) or was not cast (HIT_INVALID) have defined values: depth +inf (f32) / 0 (8-bit), normal, albedo and id black;
emission shows what the records hold (the sky colour for NONE, black for INVALID).  Alpha is 255 everywhere, as in a frame.
"""
import numpy as np

from . import abi


def _hit_mask(hits):
    k = hits["kind"]
    return (k != abi.HIT_NONE) & (k != abi.HIT_INVALID)


def _rgba(rgb8):
    out = np.empty(rgb8.shape[:-1] + (4,), dtype=np.uint8)
    out[..., :3] = rgb8
    out[..., 3] = 255
    return out


def color_map(rgb):
    """The library's colour mapping of a linear RGB value (shader.wgsl:137-151): sqrt gamma, clamp to [0, 1], 8 bits by
    truncation of c * 255.999 -- applied per channel to an (..., 3) f32 array; returns uint8."""
    c = np.asarray(rgb, dtype=np.float32)
    g = np.where(c > 0, np.sqrt(np.maximum(c, np.float32(0)), dtype=np.float32), np.float32(0)).astype(np.float32)
    g = np.minimum(np.maximum(g, np.float32(0)), np.float32(1))   # (NaN -> 0 through the where above)
    return (g * np.float32(255.999)).astype(np.uint32).astype(np.uint8)


def hash_to_color(n):
    """shader.wgsl:394-400 on a uint32 array: (..., 3) f32."""
    h = (np.asarray(n, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    r = (h % np.uint64(41)).astype(np.float32) / np.float32(40.0)
    g = (h % np.uint64(29)).astype(np.float32) / np.float32(28.0)
    b = (h % np.uint64(19)).astype(np.float32) / np.float32(18.0)
    return np.stack([r, g, b], axis=-1).astype(np.float32)


def depth(hits):
    """t per pixel as f32; +inf where nothing was hit."""
    return np.where(_hit_mask(hits), hits["t"], np.float32(np.inf)).astype(np.float32)


def depth_u8(hits, near=None, far=None):
    """Depth normalised to 8 bits, near = 255 ... far = 1, no hit = 0 (RGBA8, grey).  ``near`` / ``far`` default to the
    smallest / largest t among the hits."""
    m = _hit_mask(hits)
    t = hits["t"].astype(np.float64)
    g = np.zeros(hits.shape, dtype=np.uint8)
    if m.any():
        lo = float(t[m].min()) if near is None else float(near)
        hi = float(t[m].max()) if far is None else float(far)
        x = np.clip((t - lo) / (hi - lo), 0.0, 1.0) if hi > lo else np.zeros_like(t)
        g = np.where(m, np.rint(255.0 - 254.0 * x), 0).astype(np.uint8)
    return _rgba(np.stack([g, g, g], axis=-1))


def normal(hits):
    """(n * 0.5 + 0.5) as RGB8 (rounded to nearest); black where nothing was hit."""
    n = hits["normal"].astype(np.float32)
    c = np.rint(np.clip(n * np.float32(0.5) + np.float32(0.5), 0, 1) * 255.0).astype(np.uint8)
    c[~_hit_mask(hits)] = 0
    return _rgba(c)


def albedo(hits, surfaces):
    c = color_map(surfaces["albedo"])
    c[~_hit_mask(hits)] = 0
    return _rgba(c)


def emission(hits, surfaces):
    return _rgba(color_map(surfaces["emissive"]))


def _id_image(hits, ids):
    c = color_map(hash_to_color(ids.astype(np.uint32) + np.uint32(1)))
    c[~_hit_mask(hits) | (ids == abi.NO_INDEX)] = 0
    return _rgba(c)


def primitive_id(hits):
    """hash_to_color(prim + 1), the shader's colour-hash convention; ground / no hit black."""
    return _id_image(hits, hits["prim"])


def mesh_id(hits):
    """hash_to_color(mesh + 1) for triangle hits; everything else black."""
    return _id_image(hits, hits["mesh"])


NAMES = ("depth", "normal", "albedo", "emission", "id")


def image(name, hits, surfaces=None):
    """The RGBA8 image ``--aov name`` writes."""
    if name == "depth":
        return depth_u8(hits)
    if name == "normal":
        return normal(hits)
    if name == "id":
        return primitive_id(hits)
    if name in ("albedo", "emission"):
        if surfaces is None:
            raise ValueError(f"{name} needs the surface records")
        return albedo(hits, surfaces) if name == "albedo" else emission(hits, surfaces)
    raise ValueError(f"unknown AOV {name!r}: one of {', '.join(NAMES)}")
