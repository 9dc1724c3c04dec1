"""Scenes for the lightmap tests: a handful of hand-placed triangles given by their uvs, random convex
quads, the cube example and the 578-triangle mesh with a planar unwrap.  No device, no library."""
import os

import numpy as np

from renderbaby_amd import abi, scene_io, scenes

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def uv_triangles(uv_tris, meshes=None, shared=False):
    """(abi.GPU_TRIANGLE[m], uvs float32[]) from m triangles given as three (u, v) pairs each.  The positions lie on a tilted
    plane over the uvs -- v = (3 u - 1, 0.5 + 0.25 u + 0.5 v, 2 v - 4) --, so every triangle with uv area has a normal.
    ``shared``: equal uv pairs get one index, as an indexed mesh has them; else three fresh indices per triangle."""
    uv = np.asarray(uv_tris, f32).reshape(-1, 3, 2)
    m = len(uv)
    tris = np.zeros(m, dtype=abi.GPU_TRIANGLE)
    with np.errstate(all="ignore"):
        pos = np.stack([3 * uv[..., 0] - 1, 0.5 + 0.25 * uv[..., 0] + 0.5 * uv[..., 1], 2 * uv[..., 1] - 4], axis=-1).astype(f32)
    pos[~np.isfinite(pos)] = 0.5
    tris["v0"], tris["v1"], tris["v2"] = pos[:, 0], pos[:, 1], pos[:, 2]
    tris["mesh_index"] = 0 if meshes is None else np.asarray(meshes, np.uint32)
    if shared:
        keys, table, idx = {}, [], np.zeros((m, 3), np.uint32)
        for t in range(m):
            for k in range(3):
                key = uv[t, k].tobytes()
                if key not in keys:
                    keys[key] = len(table)
                    table.append(uv[t, k])
                idx[t, k] = keys[key]
        uvs = np.asarray(table, f32).reshape(-1)
    else:
        idx = np.arange(3 * m, dtype=np.uint32).reshape(m, 3)
        uvs = uv.reshape(-1).copy()
    tris["v0_index"], tris["v1_index"], tris["v2_index"] = idx[:, 0], idx[:, 1], idx[:, 2]
    return tris, uvs


def convex_quad(rng, lo=0.03, hi=0.97):
    """four uv corners of a convex quad inside [lo, hi]^2, counter-clockwise in uv: points of an ellipse at sorted angles"""
    while True:
        c = rng.uniform(0.35, 0.65, 2)
        r = rng.uniform(0.35, 1.0, 2) * np.minimum(c - lo, hi - c)
        ang = np.sort(rng.uniform(0, 2 * np.pi, 4))
        gaps = np.diff(np.concatenate([ang, ang[:1] + 2 * np.pi]))
        if gaps.min() > 0.3 and gaps.max() < np.pi - 0.2:
            return (c + r * np.stack([np.cos(ang), np.sin(ang)], axis=1)).astype(f32)


def quad_triangles(q, diagonal, clockwise):
    """the two triangles of quad q split along diagonal 0 (q0-q2) or 1 (q1-q3), and the shared edge's two ends"""
    if diagonal == 0:
        t, e = [(q[0], q[1], q[2]), (q[0], q[2], q[3])], (q[0], q[2])
    else:
        t, e = [(q[1], q[2], q[3]), (q[1], q[3], q[0])], (q[1], q[3])
    if clockwise:
        t = [(a, c, b) for a, b, c in t]
    return t, e


def special_triangles():
    """The hand-placed cases of the generator test, uvs for a 64 x 64 atlas (an exact power of two: u * 64 is exact), with the
    mesh index of each.  Texel centres lie at (k + 0.5) / 64."""
    s = 1.0 / 64.0
    c = lambda x, y: (x * s, 1.0 - y * s)   # noqa: E731  texel coordinates (x right, y down) -> uv
    cases = [
        ("whole atlas, box clamped", [(-1.0, -1.0), (3.0, -1.0), (-1.0, 3.0)], 0),
        ("wholly outside, uv > 1", [(1.2, 1.3), (1.9, 1.2), (1.5, 1.8)], 0),
        ("wholly outside, uv < 0", [(-0.9, -0.2), (-0.1, -0.3), (-0.5, -0.8)], 0),
        ("partly outside", [(0.8, 0.4), (1.4, 0.5), (0.9, 0.9)], 0),
        ("clockwise", [c(3, 3), c(3, 20), c(20, 3)], 0),
        ("counter-clockwise", [c(23, 23), c(40, 23), c(23, 40)], 0),
        ("zero uv area", [c(5, 50), c(10, 55), c(15, 60)], 0),
        ("a NaN uv", [(np.nan, 0.5), (0.6, 0.5), (0.5, 0.6)], 0),
        ("centres on an edge and on vertices", [c(40.5, 4.5), c(50.5, 4.5), c(40.5, 14.5)], 0),
        ("its neighbour across the diagonal", [c(50.5, 4.5), c(50.5, 14.5), c(40.5, 14.5)], 0),
        ("smaller than a texel, a centre inside", [c(30.3, 50.3), c(30.8, 50.4), c(30.4, 50.8)], 0),
        ("smaller than a texel, no centre inside", [c(33.6, 50.6), c(33.9, 50.7), c(33.7, 50.9)], 0),
        ("overlapping, first", [c(44, 40), c(60, 40), c(44, 56)], 0),
        ("overlapping, second", [c(48, 36), c(62, 50), c(48, 60)], 0),
        ("the other mesh", [c(2, 30), c(18, 34), c(6, 46)], 1),
        ("the other mesh, over the first", [c(46, 42), c(58, 44), c(50, 54)], 1),
    ]
    names = [n for n, _, _ in cases]
    return names, [t for _, t, _ in cases], [m for _, _, m in cases]


def many_triangles(m, seed=5):
    """m small random triangles spread over the atlas, either winding, for the triangle counts 1, 63, 65, 130"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.05, 0.95, (m, 1, 2))
    return (c + rng.uniform(-0.12, 0.12, (m, 3, 2))).astype(f32)


def with_mesh(scene, tris, uvs, n_meshes=1, sky=(0.5, 0.7, 1.0)):
    """`scene` with its mesh replaced by `tris` / `uvs` (one white diffuse material per mesh index) under a plain sky"""
    groups_mat = scenes.material(diffuse=(0.8, 0.8, 0.8))
    meshes = np.zeros(n_meshes, dtype=abi.MESH)
    for i in range(n_meshes):
        meshes[i]["material"] = groups_mat
        sel = np.nonzero(tris["mesh_index"] == i)[0]
        meshes[i]["triangle_index_start"], meshes[i]["triangle_count"] = (sel[0] if len(sel) else 0), len(sel)
    from renderbaby_amd import bvh
    nodes, indices = bvh.build(tris)
    u = scene.uniforms.copy()
    u["bvh_node_count"], u["bvh_triangle_count"], u["sky_color"], u["ground_enabled"] = len(nodes), len(tris), sky, 0
    return scenes.Scene(u, scene.spheres, scene.lights, meshes, nodes, indices, tris, np.asarray(uvs, f32), [], scene.name + " remeshed")


def uv_scene(tris, uvs, n_meshes=1):
    """a scene that holds nothing but the given triangles, under a sky"""
    return with_mesh(scenes.sky_only(width=16, height=8), tris, uvs, n_meshes)


def cube_scene(**kw):
    """examples/cube_scene: a textured cube (its two z faces carry the uvs 0 .. 1, the lamp faces none), two spheres, a light"""
    return scene_io.load_scene(os.path.join(ROOT, "examples", "cube_scene", "scene.json"), total_samples=1, **kw).with_params(width=32, height=24)


def mesh578():
    """the 578-triangle terrain-and-blob mesh of the radiance tests with a planar unwrap: uv = the x and z of every vertex scaled
    into 0.02 .. 0.98 (the mesh carries no uvs of its own).  The terrain is a height field, so it unwraps without overlap; the
    blob's triangles lie over it in uv and lose to the lower indices or win by theirs -- owners decide."""
    s = scenes.mesh_scene(12, 12, 32, 20, 1, 4, seed=3)
    t = s.bvh_triangles.copy()
    assert len(t) == 578
    v = np.stack([t["v0"], t["v1"], t["v2"]], axis=1)   # (m, 3, 3)
    lo, hi = v[..., [0, 2]].min((0, 1)), v[..., [0, 2]].max((0, 1))
    uv = (0.02 + 0.96 * (v[..., [0, 2]] - lo) / (hi - lo)).astype(f32)
    idx = np.arange(3 * len(t), dtype=np.uint32).reshape(-1, 3)
    t["v0_index"], t["v1_index"], t["v2_index"] = idx[:, 0], idx[:, 1], idx[:, 2]
    return scenes.Scene(s.uniforms, s.spheres, s.lights, s.meshes, s.bvh_nodes, s.bvh_indices, t, uv.reshape(-1).copy(), s.textures, "mesh578 unwrapped")
