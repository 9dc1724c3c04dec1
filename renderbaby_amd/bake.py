"""Baking and free cameras on top of ``Engine.trace_rays`` (rb_trace_rays): the engine answers
"what radiance does trace_ray return along this ray?", everything else here is numpy on the caller's side.

``irradiance``   mean radiance over cosine-weighted directions about a normal: lightmap texels, vertices, probes
``irradiance_device``  the same with the rays made and the samples summed on the device (Engine.trace_hemisphere; section 16)
``lightmap``     a mesh's lightmap in one call: surfels from its uvs, traced and resolved on the device (Engine.bake_lightmap; section 17)
``direct_irradiance``  what reaches points directly from the lights, by shadow rays to the scene's emitters (Engine.direct_light; section 21)
``lightmap_direct``    a lightmap of that direct light alone: surfels and shadow rays on the device, then the resolve
``probes``       irradiance probes: the SH9 radiance coefficients at points in free space, traced and projected on the device
                 (Engine.bake_probes; section 18)
``probe_grid``   a regular grid of probes baked and turned into the coefficients Engine.light_points blends (section 19)
``lightmap_texture``  a baked map as an RGBA8 texture that sample_texture decodes back
``camera_rays``  the rays of cameras the reference's Camera struct cannot express: equirect, ortho, thin_lens
``render_rays``  rays -> tone-mapped RGBA8 pixels, the reference's colour mapping applied to sum / weight
``render_camera``  an abi.CAMERA_EX camera (camera.make) -> RGBA8 pixels, every sample's ray made on the device with jitter and
                 a lens point of its own (Engine.trace_camera, rb_trace_camera)
"""
import numpy as np

from . import abi, aov

f32 = np.float32
KINDS = ("equirect", "ortho", "thin_lens")


def _unit(v):
    v = np.asarray(v, f32)
    return (v / np.sqrt((v[..., 0:1] * v[..., 0:1] + v[..., 1:2] * v[..., 1:2]) + v[..., 2:3] * v[..., 2:3], dtype=f32)).astype(f32)


def irradiance_rays(points, normals, samples, seed=0):
    """The rays of ``irradiance``: ``samples`` cosine-weighted directions about each unit normal (aov.cosine_directions, the
    generator of ``aov.ambient_occlusion``), from the point moved off the surface along the normal as it is there.  Returns
    (origins (m * samples, 3), directions (m * samples, 3)), numpy float32, a point's rays next to each other."""
    p = np.asarray(points, f32).reshape(-1, 3)
    n = _unit(np.asarray(normals, f32).reshape(-1, 3))
    if len(p) != len(n):
        raise ValueError("points and normals differ in length")
    reach = np.sqrt((p * p).sum(-1, keepdims=True), dtype=f32)
    org = (p + n * (f32(1e-3) * np.maximum(f32(1.0), reach))).astype(f32)   # off the surface: beyond the rounding of the point
    return np.repeat(org, samples, axis=0), aov.cosine_directions(n, samples, seed).reshape(-1, 3)


def irradiance(engine, points, normals, samples, seed=0):
    """Mean radiance arriving at each point over the cosine-weighted hemisphere about its normal -- the irradiance divided by
    pi -- as float32 (m, 3).  One ray per (point, sample), each traced once (``samples=1`` per ray) with an id of its own
    (``seed`` * m * samples + its index, 32 bits), averaged here in float32 in sample order."""
    samples = int(samples)
    if samples < 1:
        raise ValueError("samples must be at least 1")
    org, dirs = irradiance_rays(points, normals, samples, seed)
    m = len(org) // samples
    ids = ((np.arange(len(org), dtype=np.uint64) + np.uint64(seed) * np.uint64(len(org))) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    rad = engine.trace_rays(org, dirs, seeds=ids, samples=1)
    c = rad["sum"].reshape(m, samples, 3)
    total = np.zeros((m, 3), f32)
    for k in range(samples):
        total = (total + c[:, k]).astype(f32)
    return (total / f32(samples)).astype(f32)


def irradiance_device(engine, points, normals, samples, first_sample=0, seeds=None, offset=1e-3):
    """``irradiance`` with the rays made on the device (Engine.trace_hemisphere, rb_trace_hemisphere):
    m points and normals in, m sums out, summed on the device in sample order.  The directions are those of the device's
    generator (``hemisphere.rays``), not ``aov.cosine_directions``', so the result agrees with ``irradiance`` within
    Monte-Carlo noise, not bit for bit.  numpy arrays -> float32 (m, 3); torch tensors on the engine's device -> an (m, 3)
    tensor there, and nothing crosses to the host.  A point without a valid sample is 0 0 0."""
    rad = engine.trace_hemisphere(points, normals, samples, first_sample=first_sample, seeds=seeds, offset=offset)
    if isinstance(rad, np.ndarray):
        w = rad["weight"][:, None].astype(f32)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(w > 0, rad["sum"].astype(f32) / w, f32(0)).astype(f32)
    w = rad[:, 3:4]
    return (rad[:, 0:3] / w.clamp(min=1.0)) * (w > 0)


def lightmap(engine, width, height, samples, first_sample=0, mesh=None, flip=False, offset=1e-3, dilate=2):
    """The lightmap of the engine's scene over its uvs (Engine.bake_lightmap, rb_bake_lightmap): float32
    (height, width, 4), row 0 on top as sample_texture reads a texture; rgb = the mean radiance over the cosine-weighted
    hemisphere of every texel's surfel (the irradiance over pi), fourth component 0 = empty, 1 = baked, 2 = filled from its
    neighbours.  No surfel and no ray exists on the host."""
    return engine.bake_lightmap(width, height, samples, first_sample=first_sample, mesh=mesh, flip=flip, offset=offset, dilate=dilate)


def _mean(rad):
    """sum / weight of abi.RADIANCE records or of an (m, 4) tensor of them; a record without weight is 0 0 0"""
    if isinstance(rad, np.ndarray):
        w = rad["weight"][:, None].astype(f32)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(w > 0, rad["sum"].astype(f32) / w, f32(0)).astype(f32)
    w = rad[:, 3:4]
    return (rad[:, 0:3] / w.clamp(min=1.0)) * (w > 0)


def direct_irradiance(engine, points, normals, samples, emitters=None, first_sample=0, seeds=None, offset=1e-3, shorten=1e-3,
                      mask=abi.MASK_ALL, pick="uniform"):
    """What reaches each point directly from the lights, over pi, as float32 (m, 3): ``samples`` shadow rays per point towards
    points drawn on the scene's emitters (Engine.direct_light, rb_direct_light) -- the first bounce of
    ``irradiance_device`` with far less noise where the lights are small, and none of its further bounces or its sky.
    ``emitters``: an abi.EMITTER table of the caller's instead of the scene's.  numpy arrays -> float32 (m, 3); torch tensors on
    the engine's device -> an (m, 3) tensor there.  A point without a valid sample is 0 0 0.  ``pick``: Engine.direct_light's --
    "uniform", "power" (emitters picked in proportion to emission times area: the same mean with less noise where the lights
    differ), a caller's table of weights (section 23), or ("grid", grid[, tables]): a table per cell of a grid, weighted by
    power over squared distance to the cell (section 24; ``pick_grid`` makes such a grid); or ("learned", grid, rounds, samples):
    such tables times the visibility ``learn_grid`` observes at these points first, over ``rounds`` x ``samples`` training
    samples that lie behind the rendered range and are not rendered (section 25)."""
    if isinstance(pick, tuple) and len(pick) > 0 and pick[0] == "learned":
        from . import engine as _engine
        pick = _learned(engine, pick, _engine.surfel_records(points, normals), samples, emitters=emitters, first_sample=first_sample,
                        seeds=seeds, offset=offset, shorten=shorten, mask=mask)
    return _mean(engine.direct_light(points, normals, samples, emitters=emitters, first_sample=first_sample, seeds=seeds, offset=offset,
                                     shorten=shorten, mask=mask, pick=pick))


def pick_grid(emitters, counts, points=None):
    """The abi.PROBE_GRID of ``counts`` = (nx, ny, nz) cells over the bounding box of an abi.EMITTER table -- the spheres
    ``direct.emitter_bounds`` puts about its records -- and, if given, (m, 3) ``points``: what ``pick=("grid", grid)`` and
    Engine.emitter_grid take.  An axis along which the box is flat gets a cell of size 1."""
    from . import direct, probes
    ce, re = direct.emitter_bounds(emitters)
    ok = np.isfinite(ce).all(1) & np.isfinite(re)
    lo = [ce[ok] - re[ok, None]] + ([] if points is None else [np.asarray(points, np.float32).reshape(-1, 3)])
    hi = [ce[ok] + re[ok, None]] + lo[1:]
    lo, hi = np.concatenate(lo).astype(np.float64), np.concatenate(hi).astype(np.float64)
    if not len(lo):
        raise ValueError("pick_grid: neither emitters nor points to span a box")
    lo, hi = lo.min(0), hi.max(0)
    hi = np.where(hi > lo, hi, lo + 1.0)
    g = probes.grid_params(lo, hi, counts)
    g["origin"] = lo   # the counts count cells: the origin is the box's corner, not the first cell's centre
    return g


def learn_grid(engine, grid, surfels, rounds, samples, prior=1.0, emitters=None, first_sample=1 << 20, seeds=None, offset=1e-3,
               shorten=1e-3, mask=abi.MASK_ALL):
    """Pick tables per grid cell that have learned which emitters the surfels see: ``rounds`` training-only
    calls of Engine.direct_light(tally=...) over ``surfels`` (abi.SURFEL records, or a tensor of them), ``samples`` samples each
    -- round r draws samples ``first_sample`` + r ``samples`` ... --, round 0 on section 24's tables and every later round on
    the tables of the round before, all adding to one running tally; after each round Engine.emitter_grid(tally=..., prior=...)
    makes the next tables.  -> (tables, tally) as the engine's forms return them: numpy arrays for numpy surfels, tensors on
    the engine's device for a tensor.  The tables are unbiased for any samples that did not go into their tally: render with
    a sample range the training did not use.  ``rounds`` = 0: section 24's tables and an empty tally."""
    from . import engine as _engine
    rounds, samples, first_sample = int(rounds), int(samples), int(first_sample)
    if rounds < 0 or samples < 1 or first_sample + rounds * samples > 2 ** 32:
        raise ValueError("learn_grid: rounds >= 0, samples >= 1, and the training samples must end within 32 bits")
    g, rows = _engine.grid_records(grid)
    on_device = _engine.is_tensor(surfels)
    n_emit = len(engine.scene_emitters()) if emitters is None else len(emitters)
    if on_device:
        import torch
        tally = torch.zeros((rows * n_emit, 2), dtype=torch.int32, device=surfels.device)
        given = emitters
        if emitters is not None and not _engine.is_tensor(emitters):   # staged once for all rounds
            given = _engine.upload(np.ascontiguousarray(emitters, dtype=abi.EMITTER), abi.EMITTER, engine.query_device)
        tables = engine.emitter_grid(g, emitters=given, out=torch.zeros(rows * n_emit, dtype=torch.int32, device=surfels.device))
    else:
        tally = np.zeros(rows * n_emit, dtype=abi.GRID_TALLY)
        given = emitters
        tables = engine.emitter_grid(g, emitters=given)
    for r in range(rounds):
        engine.direct_light(surfels, None, samples, emitters=given, first_sample=first_sample + r * samples, seeds=seeds, offset=offset,
                            shorten=shorten, mask=mask, out=False, pick=("grid", g, tables), tally=tally)
        tables = engine.emitter_grid(g, emitters=given, tally=tally, prior=prior, out=tables if on_device else None)
    return tables, tally


def _learned(engine, pick, surf, samples, first_sample=0, **kw):
    """``pick`` as Engine.direct_light takes it: ("learned", grid, rounds, samples[, prior]) becomes ("grid", grid, tables) with
    tables trained on the sample range behind the rendered one"""
    if not (isinstance(pick, tuple) and len(pick) > 0 and pick[0] == "learned"):
        return pick
    if len(pick) not in (4, 5):
        raise ValueError('pick: ("learned", grid, rounds, samples) or ("learned", grid, rounds, samples, prior)')
    tables, _ = learn_grid(engine, pick[1], surf, pick[2], pick[3], prior=pick[4] if len(pick) == 5 else 1.0,
                           first_sample=int(first_sample) + int(samples), **kw)
    return ("grid", pick[1], tables)


def lightmap_direct(engine, width, height, samples, emitters=None, first_sample=0, mesh=None, flip=False, offset=1e-3, shorten=1e-3,
                    mask=abi.MASK_ALL, dilate=2, pick="uniform"):
    """``lightmap`` with direct light alone: the surfels of the engine's scene over its uvs (Engine.lightmap_surfels on the
    device), ``samples`` shadow rays per texel (Engine.direct_light on the device; the stream id is the texel index), the
    resolve of the sums (lightmap_resolve) -> float32 (height, width, 4) in ``lightmap``'s layout.  No surfel is ever on the
    host; the sums cross once.  ``pick``: ``direct_irradiance``'s, ("learned", grid, rounds, samples) included: the training runs over
    the same texels, on the device."""
    from . import engine as _engine
    surf, _ = engine.lightmap_surfels(width, height, mesh=mesh, flip=flip, out=(_engine.device_new(abi.SURFEL, int(width) * int(height),
                                                                                                     engine.query_device), None))
    pick = _learned(engine, pick, surf, samples, emitters=emitters, first_sample=first_sample, offset=offset, shorten=shorten, mask=mask)
    sums = engine.direct_light(surf, None, samples, emitters=emitters, first_sample=first_sample, offset=offset, shorten=shorten, mask=mask,
                               pick=pick)
    return _engine.lightmap_resolve(_engine.download(sums, abi.RADIANCE), width, height, dilate=dilate, device=engine.query_device)


def probes(engine, pos, samples, first_sample=0, seeds=None):
    """Irradiance probes at (n, 3) points in free space (Engine.bake_probes, rb_bake_probes): the
    radiance arriving from every direction as nine spherical-harmonic coefficients per colour channel, float64 (n, 9, 3), from
    ``samples`` uniform-sphere rays per probe made, traced and projected on the device.  ``probes.irradiance`` evaluates them
    for any normal; a moving object is lit from the probes around it."""
    from . import probes as model
    sh = engine.bake_probes(pos, samples, first_sample=first_sample, seeds=seeds)
    return model.radiance_coefficients(sh if isinstance(sh, np.ndarray) else sh.cpu().numpy())


def probe_grid(engine, lo, hi, counts, samples, first_sample=0, seeds=None, visibility=False, backface_limit=0.25):
    """A regular grid of irradiance probes over the box ``lo`` .. ``hi``, ``counts`` = (nx, ny, nz) cell centres along the axes
    (``probes.grid``), baked with ``samples`` rays per probe (Engine.bake_probes) and scaled to coefficients
    (Engine.probe_coefficients).  Returns (grid, coeffs): an abi.PROBE_GRID scalar and abi.SH9[nx * ny * nz],
    x fastest -- what ``Engine.light_points`` and ``aov.probe_lit`` take.  To accumulate over calls with ``first_sample``, add
    ``Engine.bake_probes``' sums and call ``Engine.probe_coefficients`` once at the end.

    ``visibility=True`` (section 20) bakes the probes' depth maps from the same rays as well (Engine.bake_probe_depth, distances
    clipped at 1.5 cell diagonals; Engine.probe_moments), gives every probe more than ``backface_limit`` of whose rays met a
    back face -- one inside geometry -- the weight 0 before the coefficients are made, and returns (grid, coeffs, moments):
    what ``Engine.light_points_visible`` takes."""
    from . import probes as model
    grid = model.grid_params(lo, hi, counts)
    pos = model.grid(lo, hi, counts)
    sh = engine.bake_probes(pos, samples, first_sample=first_sample, seeds=seeds)
    if not visibility:
        return grid, engine.probe_coefficients(sh)
    reach = 1.5 * float(np.sqrt((grid["step"].astype(np.float64) ** 2).sum()))
    maps, share = engine.probe_moments(engine.bake_probe_depth(pos, samples, reach, first_sample=first_sample, seeds=seeds))
    sh["weight"][share > np.float32(backface_limit)] = 0
    return grid, engine.probe_coefficients(sh), maps


def lightmap_texture(rgba):
    """A baked map (height, width, 4) as an RGBA8 texture, uint32 (height, width), that sample_texture (shader.wgsl:181-190)
    decodes back: byte = round(255 c^(1 / 2.2)) of c clipped to 0 .. 1, R in the low byte; alpha 255 where the texel is baked
    or filled, 0 where it is empty.  Host numpy, not bit-pinned."""
    m = np.asarray(rgba, f32)
    if m.ndim != 3 or m.shape[2] != 4:
        raise ValueError("rgba: a (height, width, 4) map is needed")
    c = np.rint(255.0 * np.clip(np.nan_to_num(m[..., :3].astype(np.float64)), 0.0, 1.0) ** (1.0 / 2.2)).astype(np.uint32)
    a = np.where(m[..., 3] != 0, np.uint32(255), np.uint32(0)).astype(np.uint32)
    return (c[..., 0] | (c[..., 1] << np.uint32(8)) | (c[..., 2] << np.uint32(16)) | (a << np.uint32(24))).astype(np.uint32)


def camera_rays(kind, width, height, pos, dir=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), ortho_width=2.0, fov_deg=60.0,
                aperture=0.0, focus_distance=1.0, seed=0):
    """(origins, directions) of a ``width`` x ``height`` image, float32 (height, width, 3), row 0 on top, column 0 on the left
    as the viewer sees it; unit directions.  ``kind``:

    equirect   the full sphere from ``pos``: column -> longitude (the centre column looks along ``dir``, longitude grows to
               the right), row -> latitude (top row up); pixel centres, so no ray points exactly at a pole
    ortho      parallel rays along ``dir`` from a window ``ortho_width`` wide centred on ``pos``
    thin_lens  a pinhole of vertical field of view ``fov_deg`` whose rays start on a lens of diameter ``aperture`` (seeded
               uniform samples on the disc, one per pixel) and meet their pixel's pinhole ray at ``focus_distance`` along it
    """
    w, h = int(width), int(height)
    if w < 1 or h < 1:
        raise ValueError("width and height must be at least 1")
    if kind not in KINDS:
        raise ValueError(f"unknown camera {kind!r}: one of {', '.join(KINDS)}")
    pos = np.asarray(pos, f32).reshape(3)
    fwd = _unit(np.asarray(dir, f32).reshape(3))
    right = np.cross(fwd, np.asarray(up, f32).reshape(3)).astype(f32)
    if not np.any(right):
        raise ValueError("dir and up are parallel")
    right = _unit(right)
    upv = np.cross(right, fwd).astype(f32)
    sx = ((np.arange(w, dtype=f32) + f32(0.5)) / f32(w) * f32(2.0) - f32(1.0))[None, :, None]    # -1 .. 1, left to right
    sy = (f32(1.0) - (np.arange(h, dtype=f32) + f32(0.5)) / f32(h) * f32(2.0))[:, None, None]    # 1 .. -1, top to bottom
    if kind == "equirect":
        lon, lat = sx * f32(np.pi), sy * f32(np.pi / 2)
        d = (np.cos(lat) * np.sin(lon)) * right + np.sin(lat) * upv + (np.cos(lat) * np.cos(lon)) * fwd
        return np.broadcast_to(pos, (h, w, 3)).astype(f32), _unit(d.astype(f32))
    if kind == "ortho":
        half_w = f32(ortho_width) / f32(2.0)
        half_h = half_w * f32(h) / f32(w)
        org = pos + (sx * half_w) * right + (sy * half_h) * upv
        return org.astype(f32), np.broadcast_to(fwd, (h, w, 3)).astype(f32)
    th = f32(np.tan(np.radians(fov_deg) / 2.0))
    d = _unit(((sx * th * f32(w) / f32(h)) * right + (sy * th) * upv + fwd).astype(f32))
    focus = pos + f32(focus_distance) * d
    rng = np.random.Generator(np.random.PCG64(seed))
    r = (f32(aperture) / f32(2.0)) * np.sqrt(rng.random((h, w, 1), dtype=f32), dtype=f32)
    phi = f32(2.0 * np.pi) * rng.random((h, w, 1), dtype=f32)
    org = (pos + (r * np.cos(phi)) * right + (r * np.sin(phi)) * upv).astype(f32)
    return org, _unit((focus - org).astype(f32))


def tone_map(radiance):
    """sum / weight per ray -> RGBA8: the reference's x / (x + 1) and colour mapping (shader.wgsl:716-722, aov.color_map);
    a ray without weight (an invalid one) is black.  ``radiance``: abi.RADIANCE of any shape."""
    w = radiance["weight"][..., None].astype(f32)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(w > 0, radiance["sum"].astype(f32) / w, f32(0)).astype(f32)
        mapped = (mean / (mean + f32(1.0))).astype(f32)
    out = np.empty(mean.shape[:-1] + (4,), dtype=np.uint8)
    out[..., :3] = aov.color_map(mapped)
    out[..., 3] = 255
    return out


def render_rays(engine, origins, dirs, samples, first_sample=0):
    """The image of a ray per pixel: (h, w, 3) origins and directions -> uint8 (h, w, 4); pixel (row, column) gets the id
    row * w + column, so two renders of one size draw the same random numbers."""
    o = np.asarray(origins, f32)
    rad = engine.trace_rays(o.reshape(-1, 3), np.asarray(dirs, f32).reshape(-1, 3), samples=samples, first_sample=first_sample)
    return tone_map(rad.reshape(o.shape[:-1]))


def render_camera(engine, cam, samples, first_sample=0):
    """The image of an abi.CAMERA_EX camera: uint8 (height, width, 4), row 0 on top, column 0 on the left.  Unlike
    ``camera_rays`` + ``render_rays``, which trace one fixed ray per pixel ``samples`` times, every sample has a ray of its own:
    edges are anti-aliased and a thin lens blurs what is off its focal plane."""
    c = np.asarray(cam, dtype=abi.CAMERA_EX).reshape(())
    rad = engine.trace_camera(c, samples, first_sample=first_sample)
    return tone_map(rad.reshape(int(c["height"]), int(c["width"])))
