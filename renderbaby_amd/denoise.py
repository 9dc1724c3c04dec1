"""The edge-avoiding a-trous denoiser of DESIGN.md section 13, restated in numpy float32: no device, no library.

``filter`` is the host model the device kernels (csrc/rb_denoise.hip) are held to bit for bit: every arithmetic step is one
IEEE binary32 operation in the order section 13 fixes -- numpy's float32 ``+ - * /`` and ``sqrt`` are correctly rounded and
never contracted.  "max(a, b)" is ``a if a > b else b`` throughout (a NaN first operand yields b).  All arrays are in the
orientation of the delivered frame (row-major, top row first, x mirrored).
"""
import numpy as np

from . import abi, aov

f32 = np.float32
TAP_H = (f32(0.375), f32(0.25), f32(0.0625))   # h[|d|] = 3/8, 1/4, 1/16


def default_params():
    """rb_denoise_default_params as an abi.DENOISE_PARAMS scalar (DESIGN.md section 13 records why these)."""
    p = np.zeros((), dtype=abi.DENOISE_PARAMS)
    p["iterations"], p["normal_power_log2"] = 3, 3
    p["sigma_depth"], p["sigma_color"], p["albedo_floor"] = 0.02, 0.0, 0.01
    return p


def params(**kw):
    """The defaults with the named fields replaced."""
    p = default_params()
    for k, v in kw.items():
        p[k] = v
    return p


def check_params(p):
    """The library's validation (RB_ERR_INVALID_OPTIONS there, ValueError here)."""
    p = np.asarray(p, dtype=abi.DENOISE_PARAMS).reshape(())
    sd, sc, af = float(p["sigma_depth"]), float(p["sigma_color"]), float(p["albedo_floor"])
    if int(p["iterations"]) > 8 or int(p["normal_power_log2"]) > 10:
        raise ValueError("iterations is 0..8, normal_power_log2 0..10")
    if not (np.isfinite(sd) and sd > 0 and np.isfinite(sc) and np.isfinite(af) and af > 0):
        raise ValueError("sigma_depth and albedo_floor are finite and positive, sigma_color finite")
    if int(p["flags"]) or p["_reserved"].any():
        raise ValueError("flags and the reserved words must be 0")
    return p


def mean_radiance(accumulation):
    """acc.xyz / acc.w per pixel (shader.wgsl:720; 0 where acc.w == 0), mirrored in x: ``Engine.read_accumulation()`` (shader x
    order) -> the (h, w, 3) float32 colour ``filter`` takes."""
    acc = np.asarray(accumulation, dtype=f32)[:, ::-1, :]
    w = acc[..., 3:4]
    with np.errstate(all="ignore"):
        c = (acc[..., :3] / w).astype(f32)
    return np.where(w == 0, f32(0), c).astype(f32)


def guides_from_records(uniforms, hits, surfaces):
    """abi.GUIDE[h, w] from the records of ``Engine.render_hits(surfaces=True)`` and the uniforms they were cast with, by the
    rule of section 13.  ``pos`` comes from ``aov.pixel_centre_dirs``, numpy's restatement of the kernels' direction: it agrees
    with the engine's own guide buffer (``Engine.denoise_guides()``) to rounding, not bit for bit."""
    u = np.asarray(uniforms, dtype=abi.UNIFORMS).reshape(-1)[0]
    g = np.zeros(hits.shape, dtype=abi.GUIDE)
    g["normal"], g["t"], g["albedo"] = hits["normal"], hits["t"], surfaces["albedo"]
    d = aov.pixel_centre_dirs(u)
    with np.errstate(all="ignore"):
        g["pos"] = (np.asarray(u["camera"]["pos"], f32) + hits["t"].astype(f32)[..., None] * d).astype(f32)
    k = hits["kind"]
    surface = (k == abi.HIT_GROUND) | (k == abi.HIT_TRIANGLE) | (k == abi.HIT_SPHERE)
    emits = (surfaces["emissive"] > 0).any(-1)
    g["cls"] = np.where(surface & ~emits, k, 0)
    return g


def _shift(a, oy, ox, fill):
    """b[y, x] = a[y + oy, x + ox], `fill` outside"""
    h, w = a.shape[:2]
    b = np.full_like(a, fill)
    ys, yd = (slice(oy, h), slice(0, h - oy)) if oy >= 0 else (slice(0, h + oy), slice(-oy, h))
    xs, xd = (slice(ox, w), slice(0, w - ox)) if ox >= 0 else (slice(0, w + ox), slice(-ox, w))
    if abs(oy) < h and abs(ox) < w:
        b[yd, xd] = a[ys, xs]
    return b


def _dot(a, b):
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]).astype(f32)


def _gt(a, b):
    """max(a, b) of section 13: a where a > b, else b"""
    return np.where(a > b, a, b).astype(f32)


def filter(color, guides, params=None, rgba=False):   # noqa: A001  (the public name the ABI's documentation uses)
    """The filter of section 13 on ``color`` ((h, w, 3) or (h, w, 4) float32 mean radiance, the fourth component ignored) and
    ``guides`` (abi.GUIDE[h, w]).  Returns the linear output, (h, w, 4) float32 with w = 1 -- and with ``rgba`` also the RGBA8
    frame, uint8 (h, w, 4): ``color_map(out / (out + 1))``."""
    p = check_params(default_params() if params is None else params)
    c = np.ascontiguousarray(np.asarray(color, dtype=f32)[..., :3])
    g = np.asarray(guides, dtype=abi.GUIDE)
    if c.shape[:2] != g.shape or c.ndim != 3:
        raise ValueError(f"colour {c.shape} and guides {g.shape} differ")
    iterations, npow = int(p["iterations"]), int(p["normal_power_log2"])
    sigma_depth, sigma_color, floor = f32(p["sigma_depth"]), f32(p["sigma_color"]), f32(p["albedo_floor"])
    with np.errstate(all="ignore"):
        # ---- prepare
        cls = np.where(np.isfinite(c).all(-1), g["cls"], 0).astype(np.uint32)
        live = cls != 0
        modul = _gt(g["albedo"].astype(f32), floor)
        r = c.copy()
        if iterations > 0:
            r[live] = (c[live] / modul[live]).astype(f32)
        n_p, pos_p = g["normal"].astype(f32), g["pos"].astype(f32)
        den = (sigma_depth * g["t"].astype(f32)).astype(f32)
        # ---- iterations
        for i in range(iterations):
            s = 1 << i
            sigma_i = f32(sigma_color * f32(2.0 ** -i))
            sigma2 = f32(sigma_i * sigma_i)
            acc = np.zeros_like(r)
            wsum = np.zeros(cls.shape, dtype=f32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    cls_q = _shift(cls, dy * s, dx * s, 0)
                    take = live & (cls_q == cls)
                    if not take.any():
                        continue
                    r_q, n_q, pos_q = _shift(r, dy * s, dx * s, 0), _shift(n_p, dy * s, dx * s, 0), _shift(pos_p, dy * s, dx * s, 0)
                    k = f32(TAP_H[abs(dx)] * TAP_H[abs(dy)])
                    w_n = _gt(_dot(n_p, n_q), f32(0))
                    for _ in range(npow):
                        w_n = (w_n * w_n).astype(f32)
                    dist = np.abs(_dot(n_p, (pos_q - pos_p).astype(f32))).astype(f32)
                    w_z = _gt((f32(1) - (dist / den).astype(f32)).astype(f32), f32(0))
                    w = ((k * w_n).astype(f32) * w_z).astype(f32)
                    if sigma_color > 0:
                        e = (r_q - r).astype(f32)
                        w_c = (f32(1) / (f32(1) + (_dot(e, e) / sigma2).astype(f32)).astype(f32)).astype(f32)
                        w = (w * w_c).astype(f32)
                    acc = np.where(take[..., None], (acc + (w[..., None] * r_q).astype(f32)).astype(f32), acc)
                    wsum = np.where(take, (wsum + w).astype(f32), wsum)
            new = (acc / wsum[..., None]).astype(f32)
            r = np.where((live & (wsum != 0))[..., None], new, r).astype(f32)
        # ---- finish
        out = np.empty(c.shape[:2] + (4,), dtype=f32)
        out[..., :3] = r
        if iterations > 0:
            out[..., :3][live] = (r[live] * modul[live]).astype(f32)
        out[..., 3] = 1
        if not rgba:
            return out
        o = out[..., :3]
        img = np.empty(c.shape[:2] + (4,), dtype=np.uint8)
        img[..., :3] = aov.color_map((o / (o + f32(1))).astype(f32))
        img[..., 3] = 255
    return out, img
