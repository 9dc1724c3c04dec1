"""The numpy model of the device's lightmap stages (csrc/rb_lightmap.hip): the same binary32 operations
in the same order, so ``owners`` / ``surfels`` equal ``rb_lightmap_surfels`` and ``resolve`` equals ``rb_lightmap_resolve`` bit
for bit.  (Where the arithmetic makes a NaN -- a surfel past the finite range, a quotient of the resolve -- its sign and payload are
numpy's here and the device's there: section 17.1.)

``prepare``      what the engine's upload makes of a triangle: v0, e1, e2 and the normal the walks report
``texel_space``  the corners A, B, C of every triangle in texels, row 0 on top
``edge``         the watertight edge function: the ends in canonical order, the sign restored afterwards
``owners``       the lowest covering triangle index of every texel, or NO_OWNER
``surfels``      (abi.SURFEL[height * width], owners): the surfel of every owned texel, zero bits elsewhere
``resolve``      abi.RADIANCE sums -> float32 (height, width, 4): sum / weight, then the fill passes round the charts
"""
import numpy as np

from . import abi
from .camera import _unit

f32, u32, u64 = np.float32, np.uint32, np.uint64
NO_OWNER = abi.LIGHTMAP_NO_OWNER
NEIGHBOURS = ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))   # (dx, dy), the order of the sums


def prepare(tris):
    """(v0, e1, e2, n), each (m, 3) float32: e1 = v1 - v0, e2 = v2 - v0, n = normalize(cross(e1, e2)) (k_prep_tris)"""
    t = np.asarray(tris, dtype=abi.GPU_TRIANGLE).reshape(-1)
    v0 = t["v0"].astype(f32)
    with np.errstate(all="ignore"):
        e1, e2 = (t["v1"] - v0).astype(f32), (t["v2"] - v0).astype(f32)
        c = np.stack([((e1[:, 1] * e2[:, 2]).astype(f32) - (e1[:, 2] * e2[:, 1]).astype(f32)).astype(f32),
                      ((e1[:, 2] * e2[:, 0]).astype(f32) - (e1[:, 0] * e2[:, 2]).astype(f32)).astype(f32),
                      ((e1[:, 0] * e2[:, 1]).astype(f32) - (e1[:, 1] * e2[:, 0]).astype(f32)).astype(f32)], axis=1)
        return v0, e1, e2, _unit(c)


def _uv_at(uvs, i):
    """uvs[i] for uint32 indices i, 0.0f where i is past the end (shader.wgsl's robust buffer access)"""
    i = np.asarray(i, u64)
    ok = i < len(uvs)
    out = np.zeros(i.shape, f32)
    out[ok] = uvs[i[ok].astype(np.int64)]
    return out


def texel_space(tris, uvs, width, height):
    """(A, B, C), each (m, 2) float32: corner k of triangle t is (u_k * float(width), (1 - v_k) * float(height)) with
    uv_k = (uv_at(2 i_k), uv_at(2 i_k + 1)), the index arithmetic in uint32"""
    t = np.asarray(tris, dtype=abi.GPU_TRIANGLE).reshape(-1)
    uvs = np.asarray(uvs, f32).reshape(-1)
    out = []
    with np.errstate(all="ignore"):
        for name in ("v0_index", "v1_index", "v2_index"):
            i = t[name].astype(u64)
            iu, iv = (i * u64(2)) & u64(0xFFFFFFFF), (i * u64(2) + u64(1)) & u64(0xFFFFFFFF)
            x = (_uv_at(uvs, iu) * f32(width)).astype(f32)
            y = ((f32(1.0) - _uv_at(uvs, iv)).astype(f32) * f32(height)).astype(f32)
            out.append(np.stack([x, y], axis=-1))
    return tuple(out)


def edge(S, T, P):
    """The value at P (..., 2) of the edge from S to T (2,): with (a, b) the ends in canonical order -- S first iff
    S.x < T.x or (S.x == T.x and S.y <= T.y) --, E = (b.x - a.x) (P.y - a.y) - (b.y - a.y) (P.x - a.x); E for ends in order,
    -E otherwise.  float32 throughout."""
    S, T, P = np.asarray(S, f32), np.asarray(T, f32), np.asarray(P, f32)
    ordered = bool(S[0] < T[0] or (S[0] == T[0] and S[1] <= T[1]))
    a, b = (S, T) if ordered else (T, S)
    with np.errstate(all="ignore"):
        dx, dy = f32(b[0] - a[0]), f32(b[1] - a[1])
        e = ((dx * (P[..., 1] - a[1]).astype(f32)).astype(f32) - (dy * (P[..., 0] - a[0]).astype(f32)).astype(f32)).astype(f32)
    return e if ordered else -e


def _box(A, B, C, width, height):
    """the texels [x0, x1] x [y0, y1] of a triangle's box cut to the atlas, or None"""
    lo = np.floor(np.minimum(np.minimum(A, B), C))
    hi = np.floor(np.maximum(np.maximum(A, B), C))
    if hi[0] < 0 or hi[1] < 0 or lo[0] > width - 1 or lo[1] > height - 1:
        return None
    return (int(max(lo[0], 0)), int(min(hi[0], width - 1)), int(max(lo[1], 0)), int(min(hi[1], height - 1)))


def _covering(tris, uvs, width, height, mesh, tri_count):
    """for every triangle that can cover a texel: (t, A, B, C, area, (x0, x1, y0, y1))"""
    t = np.asarray(tris, dtype=abi.GPU_TRIANGLE).reshape(-1)
    A, B, C = texel_space(t, uvs, width, height)
    n_valid = len(t) if tri_count is None else min(int(tri_count), len(t))
    for k in range(n_valid):
        if mesh is not None and int(t["mesh_index"][k]) != int(mesh):
            continue
        a, b, c = A[k], B[k], C[k]
        if not (np.isfinite(a).all() and np.isfinite(b).all() and np.isfinite(c).all()):
            continue
        area = edge(a, b, c)
        if not np.isfinite(area) or area == 0:
            continue
        box = _box(a, b, c, width, height)
        if box is not None:
            yield k, a, b, c, f32(area), box


def _weights(a, b, c, box):
    x0, x1, y0, y1 = box
    P = np.stack(np.meshgrid(np.arange(x0, x1 + 1, dtype=f32) + f32(0.5), np.arange(y0, y1 + 1, dtype=f32) + f32(0.5)), axis=-1)
    return edge(b, c, P), edge(c, a, P), edge(a, b, P)


def owners(tris, uvs, width, height, mesh=None, tri_count=None):
    """uint32 (height, width): the lowest index of the triangles that cover the texel's centre, NO_OWNER where none does.
    ``mesh``: only the triangles of this mesh index (None: all); ``tri_count``: triangles from this index on are skipped by the
    walks and own nothing (None: every triangle counts)."""
    own = np.full((height, width), NO_OWNER, dtype=u32)
    for k, a, b, c, area, box in _covering(tris, uvs, width, height, mesh, tri_count):
        w0, w1, w2 = _weights(a, b, c, box)
        inside = ((w0 >= 0) & (w1 >= 0) & (w2 >= 0)) if area > 0 else ((w0 <= 0) & (w1 <= 0) & (w2 <= 0))
        x0, x1, y0, y1 = box
        view = own[y0:y1 + 1, x0:x1 + 1]
        view[inside & (view > k)] = k
    return own


def barycentrics(tris, uvs, width, height, own):
    """(u, v) float32 (height, width) of every owned texel in its owner: u = w1 / area, v = w2 / area; 0 elsewhere"""
    t = np.asarray(tris, dtype=abi.GPU_TRIANGLE).reshape(-1)
    A, B, C = texel_space(t, uvs, width, height)
    u, v = np.zeros((height, width), f32), np.zeros((height, width), f32)
    for k in np.unique(own[own != NO_OWNER]):
        ys, xs = np.nonzero(own == k)
        P = np.stack([xs.astype(f32) + f32(0.5), ys.astype(f32) + f32(0.5)], axis=-1)
        a, b, c = A[k], B[k], C[k]
        area = f32(edge(a, b, c))
        with np.errstate(all="ignore"):
            u[ys, xs] = (edge(c, a, P) / area).astype(f32)
            v[ys, xs] = (edge(a, b, P) / area).astype(f32)
    return u, v


def surfels(tris, uvs, width, height, mesh=None, flip=False, tri_count=None):
    """(abi.SURFEL[height * width], uint32 owners[height * width]), texel (x, y) at y * width + x: pos = (v0 + u e1) + v e2,
    normal = the owner's prepared normal (negated with ``flip``); an unowned texel's record is all zero bits"""
    own = owners(tris, uvs, width, height, mesh, tri_count)
    u, v = barycentrics(tris, uvs, width, height, own)
    v0, e1, e2, n = prepare(tris)
    out = np.zeros(height * width, dtype=abi.SURFEL)
    o = own.reshape(-1)
    has = o != NO_OWNER
    k = o[has].astype(np.int64)
    uu, vv = u.reshape(-1)[has][:, None], v.reshape(-1)[has][:, None]
    with np.errstate(all="ignore"):
        out["pos"][has] = ((v0[k] + (uu * e1[k]).astype(f32)).astype(f32) + (vv * e2[k]).astype(f32)).astype(f32)
    out["normal"][has] = -n[k] if flip else n[k]
    return out, o.copy()


def resolve(sums, width, height, dilate=0):
    """float32 (height, width, 4) from abi.RADIANCE[height * width]: pass 0 gives {sum / weight, 1} where weight > 0 and zeros
    elsewhere; each of ``dilate`` passes then gives a texel whose fourth component is 0 the mean of its neighbours (NEIGHBOURS'
    order, inside the atlas, fourth component non-zero) of the pass before, and 2 as its fourth component."""
    s = np.asarray(sums, dtype=abi.RADIANCE).reshape(height, width)
    w = s["weight"].astype(f32)
    out = np.zeros((height, width, 4), f32)
    with np.errstate(all="ignore"):
        ok = w > 0
        out[..., :3][ok] = (s["sum"][ok] / w[ok][:, None]).astype(f32)
    out[..., 3][ok] = 1
    for _ in range(int(dilate)):
        prev = out
        pad = np.zeros((height + 2, width + 2, 4), f32)
        pad[1:-1, 1:-1] = prev
        acc = np.zeros((height, width, 3), f32)
        cnt = np.zeros((height, width), np.int64)
        for dx, dy in NEIGHBOURS:
            q = pad[1 + dy:1 + dy + height, 1 + dx:1 + dx + width]
            live = q[..., 3] != 0
            with np.errstate(all="ignore"):
                acc = np.where(live[..., None], (acc + q[..., :3]).astype(f32), acc)
            cnt += live
        fill = (prev[..., 3] == 0) & (cnt > 0)
        out = prev.copy()
        with np.errstate(all="ignore"):
            out[..., :3][fill] = (acc[fill] / cnt[fill].astype(f32)[:, None]).astype(f32)
        out[..., 3][fill] = 2
    return out
