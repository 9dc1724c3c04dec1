"""Temporal reprojection of DESIGN.md section 22, restated in numpy float32: no device, no library.

``reproject`` and ``merge`` are the host model the device kernels (csrc/rb_reproject.hip) are held to bit for bit: every
arithmetic step is one IEEE binary32 operation in the order section 22.1 fixes -- numpy's float32 ``+ - * /`` and ``sqrt`` are
correctly rounded and never contracted.  "max(a, b)" is ``a if a > b else b``, "min(a, b)" ``a if a < b else b``.  All arrays
are in the orientation of the delivered frame (row-major, top row first, x mirrored).  A frame record is four float32:
``{mean r, g, b, count}``.
"""
import numpy as np

from . import abi
from .denoise import _dot, _gt

f32 = np.float32


def default_params():
    """rb_reproject_default_params as an abi.REPROJECT_PARAMS scalar (DESIGN.md section 22.7 says where each comes from)."""
    p = np.zeros((), dtype=abi.REPROJECT_PARAMS)
    p["sigma_depth"], p["normal_min"], p["albedo_floor"], p["max_history"] = 0.02, 0.9, 0.01, 32.0
    return p


def params(**kw):
    """The defaults with the named fields replaced."""
    p = default_params()
    for k, v in kw.items():
        p[k] = v
    return p


def check_params(p):
    """The library's validation (RB_ERR_INVALID_OPTIONS there, ValueError here)."""
    p = np.asarray(p, dtype=abi.REPROJECT_PARAMS).reshape(())
    sd, nm, af, mh = (float(p[k]) for k in ("sigma_depth", "normal_min", "albedo_floor", "max_history"))
    if not (np.isfinite(sd) and sd > 0):
        raise ValueError("sigma_depth is finite and positive")
    if not (np.isfinite(nm) and -1 <= nm <= 1):
        raise ValueError("normal_min is within -1 .. 1")
    if not (np.isfinite(af) and af > 0):
        raise ValueError("albedo_floor is finite and positive")
    if not (np.isfinite(mh) and mh >= 1):
        raise ValueError("max_history is finite and at least 1")
    if int(p["flags"]) or p["_reserved"].any():
        raise ValueError("flags and the reserved words must be 0")
    return p


def view_from_camera(uniforms_or_camera, w=None, h=None):
    """rb_view_from_camera: the abi.VIEW scalar of a render camera at w x h -- the steps of a render launch (``aov.
    pixel_centre_dirs`` restates the same ones), then one operation per scalar.  An abi.UNIFORMS record brings its own size."""
    a = np.asarray(uniforms_or_camera)
    if a.dtype == abi.UNIFORMS:
        u = a.reshape(-1)[0]
        cam = u["camera"]
        w = int(u["width"]) if w is None else w
        h = int(u["height"]) if h is None else h
    else:
        cam = np.asarray(a, dtype=abi.CAMERA).reshape(-1)[0]
    w, h = int(w), int(h)
    v = np.zeros((), dtype=abi.VIEW)
    with np.errstate(all="ignore"):
        def unit(x):
            return (x / np.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2], dtype=f32)).astype(f32)

        def cross(p, q):
            return np.array([p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]], dtype=f32)
        aspect = f32(w) / f32(h)
        fwd = unit(np.asarray(cam["dir"], f32))
        right = unit(cross(np.array([0, 1, 0], f32), fwd))
        up = cross(fwd, right)
        fov = f32(cam["pane_width"]) / ((f32(2.0) * f32(cam["pane_distance"])) * aspect)
        wm1, hm1 = f32((w - 1) & 0xFFFFFFFF), f32((h - 1) & 0xFFFFFFFF)
        v["pos"], v["right"], v["up"], v["fwd"] = cam["pos"], right, up, fwd
        v["cx"] = wm1 * f32(0.5)
        v["cy"] = hm1 * f32(0.5)
        v["sx"] = v["cx"] / f32(fov * aspect)
        v["sy"] = v["cy"] / fov
    return v


def project(pos, view, w, h):
    """(X, Y, on): where the points ``pos`` (..., 3) are on a w x h screen under ``view`` (displayed column and row, float32),
    and whether section 22.1's tests let them through (z > 0, -1 < X < w, -1 < Y < h; a NaN fails)."""
    v = np.asarray(view, dtype=abi.VIEW).reshape(())
    with np.errstate(all="ignore"):
        e = (np.asarray(pos, f32) - v["pos"]).astype(f32)
        z, a, b = _dot(e, v["fwd"]), _dot(e, v["right"]), _dot(e, v["up"])
        X = (v["cx"] - ((a / z).astype(f32) * v["sx"]).astype(f32)).astype(f32)
        Y = (v["cy"] - ((b / z).astype(f32) * v["sy"]).astype(f32)).astype(f32)
        on = (z > 0) & (X > -1) & (X < f32(w)) & (Y > -1) & (Y < f32(h))
    return X, Y, on


def reproject(prev4, prev_guides, view, cur_guides, params=None):
    """REPROJECT of section 22.1: ``prev4`` (h, w, 4) float32 frame records and ``prev_guides`` abi.GUIDE[h, w] of the previous
    frame, its ``view`` (abi.VIEW), the current frame's ``cur_guides`` -> (h, w, 4) float32 history records, NONE (four +0.0)
    where the previous frame did not see the pixel's surface."""
    p = check_params(default_params() if params is None else params)
    c4 = np.ascontiguousarray(prev4, dtype=f32)
    gq, g = np.asarray(prev_guides, dtype=abi.GUIDE), np.asarray(cur_guides, dtype=abi.GUIDE)
    if c4.shape != g.shape + (4,) or gq.shape != g.shape or g.ndim != 2:
        raise ValueError(f"records {c4.shape}, previous guides {gq.shape} and current guides {g.shape} differ")
    h, w = g.shape
    sigma_depth, normal_min, floor, max_history = (f32(p[k]) for k in ("sigma_depth", "normal_min", "albedo_floor", "max_history"))
    out = np.zeros((h, w, 4), dtype=f32)
    if h * w == 0:
        return out
    with np.errstate(all="ignore"):
        cls = g["cls"]
        X, Y, on = project(g["pos"], view, w, h)
        on &= cls != 0
        Xs, Ys = np.where(on, X, f32(0)).astype(f32), np.where(on, Y, f32(0)).astype(f32)
        X0, Y0 = np.floor(Xs).astype(f32), np.floor(Ys).astype(f32)
        fx, fy = (Xs - X0).astype(f32), (Ys - Y0).astype(f32)
        ix, iy = X0.astype(np.int64), Y0.astype(np.int64)
        wx, wy = ((f32(1) - fx).astype(f32), fx), ((f32(1) - fy).astype(f32), fy)
        n_p, pos_p = g["normal"].astype(f32), g["pos"].astype(f32)
        m_p = _gt(g["albedo"].astype(f32), floor)
        den = (sigma_depth * g["t"].astype(f32)).astype(f32)
        hs = np.zeros((h, w, 3), dtype=f32)
        hn = np.zeros((h, w), dtype=f32)
        bs = np.zeros((h, w), dtype=f32)
        for dy in (0, 1):
            for dx in (0, 1):
                qx, qy = ix + dx, iy + dy
                inside = on & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                cx, cy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                bw = (wx[dx] * wy[dy]).astype(f32)
                c_q, g_q = c4[cy, cx], gq[cy, cx]
                dn = _dot(n_p, g_q["normal"].astype(f32))
                dist = np.abs(_dot(n_p, (g_q["pos"].astype(f32) - pos_p).astype(f32))).astype(f32)
                take = inside & (bw > 0) & (g_q["cls"] == cls) & np.isfinite(c_q).all(-1) & (c_q[..., 3] > 0) \
                    & (dn >= normal_min) & (dist <= den)
                m_q = _gt(g_q["albedo"].astype(f32), floor)
                r = (c_q[..., :3] / m_q).astype(f32)
                hs = np.where(take[..., None], (hs + (bw[..., None] * r).astype(f32)).astype(f32), hs)
                hn = np.where(take, (hn + (bw * c_q[..., 3]).astype(f32)).astype(f32), hn)
                bs = np.where(take, (bs + bw).astype(f32), bs)
        res = np.empty((h, w, 4), dtype=f32)
        res[..., :3] = ((hs / bs[..., None]).astype(f32) * m_p).astype(f32)
        hl = (hn / bs).astype(f32)
        res[..., 3] = np.where(hl < max_history, hl, max_history)
        keep = (bs > 0) & np.isfinite(res).all(-1)
        out[keep] = res[keep]
    return out


def merge(hist4, cur_guides, cur4):
    """MERGE of section 22.1: the history records ``hist4`` (``reproject``'s result) and the current frame's records ``cur4``
    ((h, w, 4) float32: mean radiance and sample count) -> (h, w, 4) float32.  A pass-through pixel keeps ``cur4``'s bits."""
    hst = np.ascontiguousarray(hist4, dtype=f32)
    cur = np.ascontiguousarray(cur4, dtype=f32)
    g = np.asarray(cur_guides, dtype=abi.GUIDE)
    if hst.shape != cur.shape or cur.shape != g.shape + (4,):
        raise ValueError(f"history {hst.shape}, records {cur.shape} and guides {g.shape} differ")
    with np.errstate(all="ignore"):
        n, hc = cur[..., 3], hst[..., 3]
        through = (g["cls"] == 0) | ~np.isfinite(cur).all(-1) | ~(n >= 0) | (hc == 0)
        tot = (hc + n).astype(f32)
        res = np.empty_like(cur)
        res[..., :3] = (((hst[..., :3] * hc[..., None]).astype(f32) + (cur[..., :3] * n[..., None]).astype(f32)).astype(f32) / tot[..., None]).astype(f32)
        res[..., 3] = tot
    out = cur.copy()
    out.view(np.uint32)[~through] = res.view(np.uint32)[~through]
    return out


def frame_records(accumulation):
    """The engine's current frame records from ``Engine.read_accumulation()`` (shader x order): {mean radiance of section 13.1,
    acc.w}, mirrored in x -- what rb_denoise_history merges onto its base."""
    from .denoise import mean_radiance
    acc = np.asarray(accumulation, dtype=f32)
    out = np.empty(acc.shape, dtype=f32)
    out[..., :3] = mean_radiance(acc)
    out[..., 3] = acc[:, ::-1, 3]
    return out
