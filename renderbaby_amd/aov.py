"""First-hit buffers as images: pure numpy over the records of ``Engine.render_hits`` / ``Engine.cast_rays``
(abi.HIT, abi.SURFACE).  No device, no library -- except ``ambient_occlusion``, which asks the engine one any-hit query,
``ambient_occlusion_device``, which asks it for the openness of one surfel per hit, and ``probe_lit``, which asks it to light
one surfel per hit from a baked probe grid.

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


def pixel_centre_dirs(uniforms):
    """[row, displayed column] -> the direction of the pixel-centre ray (shader.wgsl:690-709 with both offsets 0, x mirrored
    like the frame), numpy float32.  ``uniforms``: abi.UNIFORMS."""
    f32 = np.float32
    u = np.asarray(uniforms, dtype=abi.UNIFORMS).reshape(-1)[0]
    w, h = int(u["width"]), int(u["height"])

    def unit(v):
        v = np.asarray(v, f32)
        return (v / np.sqrt((v[..., 0:1] * v[..., 0:1] + v[..., 1:2] * v[..., 1:2]) + v[..., 2:3] * v[..., 2:3], dtype=f32)).astype(f32)
    aspect = f32(w) / f32(h)
    fwd = unit(u["camera"]["dir"])
    right = unit(np.cross(np.array([0, 1, 0], f32), fwd).astype(f32))
    up = np.cross(fwd, right).astype(f32)
    fov = f32(u["camera"]["pane_width"]) / (f32(2.0) * f32(u["camera"]["pane_distance"]) * aspect)
    x = (f32(w - 1) - np.arange(w, dtype=f32)) / f32(max(w - 1, 1))
    y = np.arange(h, dtype=f32) / f32(max(h - 1, 1))
    su = ((x * f32(2.0) - f32(1.0)) * aspect)[None, :, None]
    sv = (f32(1.0) - y * f32(2.0))[:, None, None]
    return unit((fov * su) * right + (fov * sv) * up + fwd)


def ambient_occlusion_rays(uniforms, hits, n_dirs=16, seed=0):
    """The rays of ``ambient_occlusion``: for every pixel whose centre ray hit something, ``n_dirs`` cosine-weighted
    directions about the normal turned towards the camera, from the hit point ``pos + t d`` moved off the surface along that
    normal.  Returns (pixel mask [rows, width], origins (m * n_dirs, 3), directions (m * n_dirs, 3)), numpy float32."""
    f32 = np.float32
    u = np.asarray(uniforms, dtype=abi.UNIFORMS).reshape(-1)[0]
    m = _hit_mask(hits)
    d = pixel_centre_dirs(u)
    if d.shape[:2] != hits.shape:
        raise ValueError(f"the records are {hits.shape}, the uniforms' frame {d.shape[:2]}")
    d, t, n = d[m], hits["t"][m].astype(f32)[:, None], hits["normal"][m].astype(f32)
    n = np.where((n * d).sum(-1, keepdims=True) > 0, -n, n).astype(f32)
    pos = (np.asarray(u["camera"]["pos"], f32) + t * d).astype(f32)
    org = (pos + n * (f32(1e-3) * np.maximum(f32(1.0), t))).astype(f32)   # off the surface: beyond the rounding of pos
    return m, np.repeat(org, n_dirs, axis=0), cosine_directions(n, n_dirs, seed).reshape(-1, 3)


def cosine_directions(normals, n_dirs, seed=0):
    """``n_dirs`` cosine-weighted directions about each of the (m, 3) unit ``normals``: (m, n_dirs, 3), numpy float32 -- the ray
    generator of ``ambient_occlusion`` and of ``bake.irradiance``."""
    f32 = np.float32
    n = np.asarray(normals, f32).reshape(-1, 3)
    rng = np.random.Generator(np.random.PCG64(seed))
    r1, r2 = rng.random((len(n), n_dirs), dtype=f32), rng.random((len(n), n_dirs), dtype=f32)
    phi, r = f32(2.0 * np.pi) * r1, np.sqrt(r2, dtype=f32)
    # a tangent frame about n (any: the distribution is symmetric about n)
    a = np.where(np.abs(n[:, 0:1]) > f32(0.5), np.array([0, 1, 0], f32), np.array([1, 0, 0], f32))
    tx = np.cross(a, n).astype(f32)
    tx /= np.sqrt((tx * tx).sum(-1, keepdims=True), dtype=f32)
    ty = np.cross(n, tx).astype(f32)
    return ((r * np.cos(phi))[..., None] * tx[:, None, :] + (r * np.sin(phi))[..., None] * ty[:, None, :]
            + np.sqrt(np.maximum(f32(1.0) - r2, f32(0)), dtype=f32)[..., None] * n[:, None, :]).astype(f32)


def ambient_occlusion(engine, hits, n_dirs=16, radius=1.0, seed=0, uniforms=None):
    """Ambient occlusion of the first hits ``engine.render_hits()`` returned: the share of ``n_dirs`` cosine-weighted
    directions per hit along which nothing lies within ``radius`` -- ONE any-hit query (Engine.occluded with tmax = radius;
    point lights are no occluders).  float32 [rows, width] in [0, 1] in the orientation of the frame: 1 = open, 0 = enclosed;
    1 where nothing was hit.  ``uniforms``: the camera, by default the uniforms the engine last accepted in an ``update``, ``render`` or ``frame_iterator``
    call -- creating an engine sends it no scene, so one of them must come first (``render_hits`` needs it anyway) or
    ``uniforms`` must be given."""
    u = engine.uniforms if uniforms is None else uniforms
    if u is None:
        raise ValueError("the engine has accepted no update yet: call update() / render() first, or pass uniforms=")
    m, org, dirs = ambient_occlusion_rays(u, hits, n_dirs, seed)
    ao = np.ones(hits.shape, dtype=np.float32)
    if len(org):
        tmax = np.full(len(org), radius, dtype=np.float32)
        occ = engine.occluded(org, dirs, tmax, abi.MASK_ALL & ~abi.MASK_LIGHTS)
        blocked = (occ.reshape(-1, n_dirs) == abi.OCCL_OCCLUDED).sum(1)
        ao[m] = np.float32(1.0) - blocked.astype(np.float32) / np.float32(n_dirs)
    return ao


def ambient_occlusion_surfels(uniforms, hits):
    """The surfels of ``ambient_occlusion_device``: for every pixel whose centre ray hit something, the hit point
    ``pos + t d`` and the normal turned towards the camera, as ``ambient_occlusion_rays`` turns it.  Returns (pixel mask
    [rows, width], points (m, 3), normals (m, 3)), numpy float32."""
    f32 = np.float32
    u = np.asarray(uniforms, dtype=abi.UNIFORMS).reshape(-1)[0]
    m = _hit_mask(hits)
    d = pixel_centre_dirs(u)
    if d.shape[:2] != hits.shape:
        raise ValueError(f"the records are {hits.shape}, the uniforms' frame {d.shape[:2]}")
    d, t, n = d[m], hits["t"][m].astype(f32)[:, None], hits["normal"][m].astype(f32)
    n = np.where((n * d).sum(-1, keepdims=True) > 0, -n, n).astype(f32)
    return m, (np.asarray(u["camera"]["pos"], f32) + t * d).astype(f32), n


def ambient_occlusion_device(engine, hits, samples=16, radius=1.0, first_sample=0, uniforms=None):
    """``ambient_occlusion`` with the directions made on the device (Engine.openness, rb_openness_hemisphere; DESIGN.md
    section 16): one surfel per hit goes up, 32 B, and two counts per hit come back -- no ray exists on the host.  The
    directions are those of the device's generator (``hemisphere.rays``), not ``cosine_directions``', so the image agrees with
    ``ambient_occlusion``'s within the noise of ``samples`` directions, not bit for bit.  float32 [rows, width]: open / valid;
    1 where nothing was hit or no sample was valid."""
    u = engine.uniforms if uniforms is None else uniforms
    if u is None:
        raise ValueError("the engine has accepted no update yet: call update() / render() first, or pass uniforms=")
    m, pts, nrm = ambient_occlusion_surfels(u, hits)
    ao = np.ones(hits.shape, dtype=np.float32)
    if len(pts):
        res = engine.openness(pts, nrm, samples, radius, first_sample=first_sample)
        valid = res["valid"].astype(np.float32)
        ao[m] = np.where(valid > 0, res["open"].astype(np.float32) / np.maximum(valid, np.float32(1)), np.float32(1)).astype(np.float32)
    return ao


def probe_lit(engine, grid, coeffs, hits, surfaces, uniforms=None, moments=None, visibility=None):
    """What a baked probe grid looks like on the scene (Engine.light_points, rb_light_points_device): the
    first hits ``engine.render_hits(surfaces=True)`` returned, lit from the grid in one launch -- ``grid``: an abi.PROBE_GRID
    scalar, ``coeffs``: its coefficient records (``bake.probe_grid`` makes both).  Linear RGB float32 [rows, width, 3] in the
    orientation of the frame, for ``color_map``: a filterable hit (the denoiser's rule: a surface that emits nothing) gives
    emission + albedo x value with the normal turned towards the camera; a light or an emitting surface its emission; a miss
    the sky, as the records hold it; a pixel the grid does not reach (weight 0) albedo x 0.  No shadows, no leaks held back:
    it shows the probes, not the scene's light.  With ``moments`` (``bake.probe_grid(visibility=True)``'s maps) the blend is
    Engine.light_points_visible's (section 20), which holds the leaks back; ``visibility``: its keyword arguments (normal_bias,
    min_visibility, wrap, depth), None for the defaults."""
    u = engine.uniforms if uniforms is None else uniforms
    if u is None:
        raise ValueError("the engine has accepted no update yet: call update() / render() first, or pass uniforms=")
    m, pts, nrm = ambient_occlusion_surfels(u, hits)
    img = surfaces["emissive"].astype(np.float32).copy()
    lit = m & (hits["kind"] != abi.HIT_LIGHT) & ~(surfaces["emissive"] > 0).any(-1)
    if len(pts):
        if moments is None and visibility is None:
            res = engine.light_points(grid, coeffs, pts, nrm)
        else:
            res = engine.light_points_visible(grid, coeffs, moments, pts, nrm, **(visibility or {}))
        value = np.zeros(hits.shape + (3,), dtype=np.float32)
        value[m] = np.where(res["weight"][:, None] > 0, res["value"], np.float32(0))
        img[lit] = (img[lit] + surfaces["albedo"][lit].astype(np.float32) * value[lit]).astype(np.float32)
    return img


def ambient_occlusion_map(engine, width, height, samples, radius, mesh=None, flip=False, first_sample=0, offset=1e-3):
    """The ambient occlusion of a mesh as a map over its uvs: the surfel of every texel of a ``width`` x
    ``height`` atlas (Engine.lightmap_surfels), then the openness of every surfel (Engine.openness) -- torch tensors on the
    engine's device from the first call to the second, so no surfel exists on the host.  float32 (height, width), row 0 on top
    as sample_texture reads a texture: open / valid; NaN where no triangle owns the texel or no sample was valid."""
    import torch
    n = int(width) * int(height)
    dev = torch.device("cuda", engine.query_device)
    surf = torch.empty((n, 8), dtype=torch.float32, device=dev)
    engine.lightmap_surfels(width, height, mesh=mesh, flip=flip, out=(surf, None))
    res = engine.openness(surf[:, 0:3].contiguous(), surf[:, 4:7].contiguous(), samples, radius, first_sample=first_sample, offset=offset)
    res = res.cpu().numpy().astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        ao = np.where(res[:, 1] > 0, res[:, 0] / res[:, 1], np.float32(np.nan)).astype(np.float32)
    return ao.reshape(int(height), int(width))


def ao_u8(ao):
    """an AO image as RGBA8 grey (rounded to nearest)"""
    g = np.rint(np.clip(ao, 0, 1) * 255.0).astype(np.uint8)
    return _rgba(np.stack([g, g, g], axis=-1))


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
