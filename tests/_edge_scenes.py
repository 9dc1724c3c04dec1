"""Scenes and rays that take texture lookup, uv interpolation, the checkerboard and the per-material prep to their edges
(plain module: no fixtures, no GPU, no oracle).  tests/test_shading_edges_scene.py shows on the oracle alone that the rays
reach what they are meant to reach; tests/test_gpu_shading_edges.py sends the same rays and frames through the library.

The wall: one unit quad (two triangles, own mesh, own material) per case in the plane z = 0, facing +z, on a 1.5 pitch;
aimed rays start at z = 3 and run along -z.  Behind it (z = -1.5) a 10 x 10 backdrop of 200 triangles with the checker
texture tiled over it, so that the tree has several nodes (the chunked walk and the library's own tree apply) and spheres
beside the wall inherit a uv too.  In front of some quads spheres (z = 0.6) and in front of two of those point lights
(z = 1.3): the inherited uv / use_texture cases of shader.wgsl:574-601.

Texture order (offsets 0, 1, 8, 13, 28, 284, 316 texels: all but the first nonzero): 1 x 1, 1 x 7, 5 x 1, 3 x 5,
16 x 16 "all bytes", the 8 x 4 checker, 257 x 3.  Every texel word has a nonzero alpha byte.
"""
import numpy as np

from renderbaby_amd import abi, scenes

f32 = np.float32
N_TEX = 7
T1X1, T1X7, T5X1, T3X5, ALL_BYTES, CHECKER, T257X3 = range(7)
PITCH, COLS = 1.5, 6
EYE_Z, SPHERE_Z, LIGHT_Z, BACK_Z = 3.0, 0.6, 1.3, -1.5
SPHERE_R, LIGHT_R = 0.25, 0.12
GROUND_HEIGHT = -1.0
LOW_EYE = (0.3, -0.5, 5.0)            # half a unit above the ground, below everything else in the scene
T = f32(0.01)                         # shader.wgsl:615-617


# -------------------------------------------------------------- textures ---
def _generic(w, h, salt):
    k = np.arange(w * h, dtype=np.uint32)
    r, g, b = (k * 29 + 7 + salt) & 255, (k * 53 + 19 + 3 * salt) & 255, (k * 11 + 201 + 5 * salt) & 255
    a = ((k * 37 + 11) & 255) | 1
    return (w, h, (r | (g << 8) | (b << 16) | (a << 24)).astype(np.uint32))


def all_bytes_texture():
    """16 x 16: texel k has R = k, G = (7 k + 3) & 255, B = 255 - k -- three permutations of 0..255"""
    k = np.arange(256, dtype=np.uint32)
    return (16, 16, (k | (((k * 7 + 3) & 255) << 8) | ((255 - k) << 16) | ((((k * 37 + 11) & 255) | 1) << 24)).astype(np.uint32))


def edge_textures():
    return [_generic(1, 1, 1), _generic(1, 7, 2), _generic(5, 1, 3), _generic(3, 5, 4), all_bytes_texture(),
            scenes.checker_texture(), _generic(257, 3, 6)]


def other_textures(n):
    """n textures of other sizes than edge_textures()' for the update tests (same indices, other offsets)"""
    dims = [(2, 3), (7, 1), (1, 1), (4, 9), (16, 16), (3, 3), (1, 5), (9, 2), (6, 6)]
    return [(all_bytes_texture() if (w, h) == (16, 16) else _generic(w, h, 40 + i)) for i, (w, h) in enumerate(dims[:n])]


# ------------------------------------------------------------- the wall ---
# (name, texture_index, (u at s = 0, u at s = 1, v at t = 0, v at t = 1), grid points per side beside the texel centres)
def _quad_specs():
    q = [("tex0", T1X1, (0.25, 0.75, 0.25, 0.75), 3)]   # (the middle of [0, 1]: uvs[0] must not be 0, or a uv guard that returns uvs[0] would pass)
    q += [(f"tex{i}", i, (0.0, 1.0, 0.0, 1.0), 3) for i in range(1, N_TEX)]
    for name, t in (("bytes", ALL_BYTES), ("3x5", T3X5)):
        q += [(f"tiled_{name}", t, (-2.5, 3.25, -2.5, 3.25), 9),
              (f"integer_{name}", t, (-1.0, 3.0, 3.0, -1.0), 9),          # corners, edge midpoints and interior points ON integers (dyadic weights: exactly)
              (f"offset_{name}", t, (1e6 + 0.5, 1e6 + 1.5, 1e6 + 1.5, 1e6 + 0.5), 9),
              (f"below_{name}", t, (-1e-9, 0.5, -1e-9, 0.5), 9),          # fract(-1e-9) rounds to 1.0: the x clamp
              (f"vzero_{name}", t, (0.1, 0.9, 0.0, 0.75), 9)]             # v = 0 exactly: (1 - v) * height == height, the y clamp
    q += [("oob_ntex", N_TEX, (0.0, 1.0, 0.0, 1.0), 3), ("oob_ntex5", N_TEX + 5, (0.0, 1.0, 0.0, 1.0), 3),
          ("oob_max", 2 ** 31 - 1, (0.0, 1.0, 0.0, 1.0), 3)]
    return q


QUADS = _quad_specs()
# the last two groups of the mesh, after the backdrop: their uv indices are the last of `uvs`, which is then cut short
TAIL_QUADS = [("uv_straddle", ALL_BYTES, (0.2, 0.8, 0.2, 0.8), 5), ("uv_beyond", ALL_BYTES, (0.3, 0.9, 0.3, 0.9), 5)]
ALL_QUADS = QUADS + TAIL_QUADS
QUAD_INDEX = {q[0]: i for i, q in enumerate(ALL_QUADS)}
# spheres in front of quads: (quad, texture_index of the sphere, has a light in front, the light's texture_index)
FRONT = [("tex3", T257X3, True, -1), ("tiled_bytes", T3X5, True, T1X7), ("tex5", -1, False, None), ("oob_ntex", ALL_BYTES, False, None),
         ("integer_3x5", ALL_BYTES, False, None)]


def quad_corner(i):
    return (i % COLS - 3) * PITCH, (i // COLS) * PITCH


def _quad_at(cx, cy, z):
    return scenes._quad((cx, cy, z), (cx + 1.0, cy, z), (cx + 1.0, cy + 1.0, z), (cx, cy + 1.0, z))   # normal +z


def _quad_uv(ua, ub, va, vb):
    return [[(ua, va), (ub, va), (ub, vb)], [(ua, va), (ub, vb), (ua, vb)]]


# ----------------------------------------------- materials at the thresholds ---
def strength(c):
    """shader.wgsl:615-616 in binary32, the kernel's order"""
    c = np.asarray(c, f32)
    return f32(f32(f32(c[0] + c[1]) + c[2]) / f32(3.0))


def _step(x, n):
    x = f32(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, f32(np.inf if n > 0 else -np.inf))
    return x


def threshold_triples():
    """{name: triple}: for the families (a, a, a), (0, 0, x) and (a, a / 2, 0), found by search over neighbouring floats, the
    triples whose strength is the largest float below 0.01f, 0.01f itself where the family reaches it, and the smallest
    above: the three values that tell `>` from `>=` and `<` from `<=`."""
    fams = {"aaa": (f32(0.01), lambda a: (a, a, a)), "00x": (f32(0.03), lambda x: (f32(0), f32(0), x)),
            "ab0": (f32(0.02), lambda a: (a, f32(a / f32(2.0)), f32(0)))}
    out = {}
    for name, (mid, make) in fams.items():
        cands = [make(_step(mid, k)) for k in range(-40, 41)]
        s = np.array([strength(c) for c in cands], f32)
        assert (np.diff(s) >= 0).all() and s[0] < T < s[-1]
        out[name + "_below"] = cands[int(np.flatnonzero(s < T)[-1])]
        out[name + "_above"] = cands[int(np.flatnonzero(s > T)[0])]
        if (s == T).any():
            out[name + "_equal"] = cands[int(np.flatnonzero(s == T)[0])]
    return out


SHININESS = [-50.0, 0.0, 1e-3, 999.99994, 1000.0, 1000.0001, 5e4, np.inf, np.nan]


def threshold_materials():
    """[(name, material)]: specular around `> 0.01f` under a zero diffuse, diffuse around `< 0.01f` under a specular of 0.5
    (textured: albedo = diffuse * texture when not metal), and every shininess of SHININESS on a plain metal."""
    out = []
    for name, c in threshold_triples().items():
        out.append(("spec_" + name, scenes.material(diffuse=(0, 0, 0), specular=c, shininess=400.0, texture_index=ALL_BYTES)))
        out.append(("diff_" + name, scenes.material(diffuse=c, specular=(0.5, 0.5, 0.5), shininess=700.0, texture_index=ALL_BYTES)))
    for sh in SHININESS:
        out.append((f"shininess_{sh}", scenes.material(diffuse=(0, 0, 0), specular=(0.8, 0.7, 0.6), shininess=sh)))
    return out


def threshold_sphere_centre(k):
    return (-5.0 + 0.5 * (k % 20), 6.5 + 0.75 * (k // 20), SPHERE_Z)


# ---------------------------------------------------------------- scene ---
def texture_edges_scene(width=64, height=48, spp=3, depth=6, color_hash=0, camera="main"):
    groups, uv_groups = [], []
    for i, (name, tex, uvr, _) in enumerate(QUADS):
        cx, cy = quad_corner(i)
        d = 0.5 + 0.4 * ((i * 5) % 7) / 7.0
        groups.append((scenes.material(diffuse=(d, 0.9, 1.0 - 0.5 * d), texture_index=tex), _quad_at(cx, cy, 0.0)))
        uv_groups.append(_quad_uv(*uvr))
    back, back_uv = [], []
    for j in range(10):
        for i in range(10):
            x, y = -6.0 + 1.2 * i, -0.25 + 1.0 * j
            back += scenes._quad((x, y, BACK_Z), (x + 1.2, y, BACK_Z), (x + 1.2, y + 1.0, BACK_Z), (x, y + 1.0, BACK_Z))
            ua, ub, va, vb = 0.37 * x, 0.37 * (x + 1.2), 0.37 * y - 1.0, 0.37 * (y + 1.0) - 1.0
            back_uv += _quad_uv(ua, ub, va, vb)
    groups.append((scenes.material(diffuse=(0.7, 0.7, 0.6), texture_index=CHECKER), back))
    uv_groups.append(back_uv)
    for k, (name, tex, uvr, _) in enumerate(TAIL_QUADS):
        cx, cy = quad_corner(len(QUADS) + k)
        groups.append((scenes.material(diffuse=(0.9, 0.8, 0.7), texture_index=tex), _quad_at(cx, cy, 0.0)))
        uv_groups.append(_quad_uv(*uvr))

    mats = threshold_materials()
    sp = np.zeros(len(FRONT) + len(mats), dtype=abi.SPHERE)
    lights = []
    for k, (qname, tex, lit, ltex) in enumerate(FRONT):
        cx, cy = quad_corner(QUAD_INDEX[qname])
        sp[k]["center"], sp[k]["radius"] = (cx + 0.5, cy + 0.5, SPHERE_Z), SPHERE_R
        sp[k]["material"] = scenes.material(diffuse=(0.9, 0.6 + 0.05 * k, 0.8), texture_index=tex)
        if lit:
            lights.append(((cx + 0.5, cy + 0.5, LIGHT_Z), ltex))
    for k, (_, m) in enumerate(mats):
        sp[len(FRONT) + k]["center"], sp[len(FRONT) + k]["radius"] = threshold_sphere_centre(k), 0.2
        sp[len(FRONT) + k]["material"] = m
    lt = np.zeros(len(lights), dtype=abi.POINT_LIGHT)
    for k, (c, ltex) in enumerate(lights):
        lt[k]["center"], lt[k]["radius"] = c, LIGHT_R
        lt[k]["material"] = scenes.material(diffuse=(0.5, 0.6, 0.7), specular=(0, 0, 0), emissive=(3.0, 2.5, 2.0), illum=0,
                                            texture_index=ltex)
    if camera == "main":
        pos, dirn = (0.0, 3.5, 16.0), (0.0, -0.05, -1.0)
    else:   # "low": grazing the ground towards +x, past the wall
        pos, dirn = LOW_EYE, (1.0, -0.01, 0.3)
    u = scenes.make_uniforms(width, height, spp, depth, cam_pos=pos, cam_dir=dirn, ground_enabled=1, ground_height=GROUND_HEIGHT,
                             checkerboard_enabled=1, sky=(0.5, 0.7, 1.0), color_hash=color_hash, cb1=(0.05, 0.05, 0.05),
                             cb2=(1.0, 0.0, 1.0))
    s = scenes._finish("texture_edges", u, sp, lt, groups, uv_groups, edge_textures())
    # cut `uvs` short (the ABI takes any length): of uv_straddle's first triangle, vertex 0 and the u of vertex 1 stay, the v of
    # vertex 1 and vertex 2 are beyond the end (so are its second triangle and all of uv_beyond)
    n_tris = len(s.bvh_triangles)
    s.uvs = np.ascontiguousarray(s.uvs[:6 * (n_tris - 4) + 3])
    return s


def quad_triangles(scene, name):
    """indices of the two triangles of a quad of the wall (build_mesh_arrays keeps the groups' order)"""
    i = QUAD_INDEX[name]
    t0 = 2 * i if i < len(QUADS) else len(scene.bvh_triangles) - 4 + 2 * (i - len(QUADS))
    return t0, t0 + 1


# ----------------------------------------------------------------- rays ---
def _quad_points(spec, textures):
    name, tex, (ua, ub, va, vb), n = spec
    pts = [(i / (n - 1), j / (n - 1)) for j in range(n) for i in range(n)]
    if 0 <= tex < len(textures) and (ua, ub, va, vb) in ((0.0, 1.0, 0.0, 1.0), (0.25, 0.75, 0.25, 0.75)):
        w, h, _ = textures[tex]   # one ray at every texel's centre: u = (x + 0.5) / w, v = 1 - (y + 0.5) / h
        pts += [(((x + 0.5) / w - ua) / (ub - ua), ((1.0 - (y + 0.5) / h) - va) / (vb - va)) for y in range(h) for x in range(w)]
    if name in [f[0] for f in FRONT]:   # a fine grid round the centre: the sphere and the light in front
        pts += [(0.5 + 0.05 * i, 0.5 + 0.05 * j) for j in range(-4, 5, 2) for i in range(-4, 5, 2)]
        pts += [(0.5 + 0.04 * i, 0.5 + 0.04 * j) for j in range(-2, 3) for i in range(-2, 3)]
    return pts


def aimed_rays(scene):
    """-> (origins, directions, quad index per ray): rays along -z at chosen points of every quad of the wall"""
    O, Q = [], []
    for qi, spec in enumerate(ALL_QUADS):
        cx, cy = quad_corner(qi)
        for s, t in _quad_points(spec, scene.textures):
            O.append((cx + s, cy + t, EYE_Z))
            Q.append(qi)
    O = np.array(O, f32)
    D = np.tile(np.array([0, 0, -1], f32), (len(O), 1))
    return O, D, np.array(Q)


def threshold_rays(scene):
    """one ray at the centre of every threshold sphere -> (origins, directions, sphere index per ray)"""
    n = len(threshold_materials())
    O = np.array([threshold_sphere_centre(k)[:2] + (EYE_Z,) for k in range(n)], f32)
    return O, np.tile(np.array([0, 0, -1], f32), (n, 1)), np.arange(n) + len(FRONT)


DY_MIN = f32(1e-6)   # shader.wgsl:403: |d.y| < 1e-6 is no ground hit


def far_ground_rays():
    """Rays that meet the ground far away, so that floor(uv * 10) leaves the range of i32 (shader.wgsl:160-163): from LOW_EYE and
    from origins high above it (the ground test wants |d.y| >= 1e-6, so t * d.x beyond 5e5 needs height), both signs of x and z,
    d.y at exactly 1e-6 and on either side of it, and origins so far out in x that uv * 10 is infinite.  Directions are NOT
    normalised (the device does that); (1, -1e-6, 0) normalises to itself.  (pos = origin + t * d with t < 1e20 is finite for a
    finite origin: an infinite uv itself cannot occur.)"""
    O, D = [], []
    x0, _, z0 = LOW_EYE
    for sx in (1.0, -1.0):
        for sz in (1.0, -1.0):
            for dz in (0.0, 0.3, 0.731, 1.0):
                # near: uv * 10 within i32, sums of both parities and signs
                for dy in (0.01, 0.0037, 0.05):
                    O.append(LOW_EYE); D.append((sx, -dy, sz * dz))
                # far: the height over the ground and the slope give t * d.x of 1e9 (saturates after * 10), 2.5e9, 1e10, 5e11, 1.5e19, 4.5e19
                # (a slope of 2e-6 stays above the ground test's 1e-6 when the direction is normalised: its length is below sqrt(2))
                for height, dy in ((1e4, 1e-5), (2.5e4, 1e-5), (1e5, 1e-5), (1e6, 2e-6), (3e13, 2e-6), (9e13, 2e-6)):
                    O.append((x0, GROUND_HEIGHT + height, z0)); D.append((sx, -dy, sz * dz))
                    O.append((x0, GROUND_HEIGHT + height, z0)); D.append((sx * dz, -dy, sz))
    for height in (0.5, 1e4, 1e6):   # the ground test's own threshold: exactly 1e-6 is a hit, one float less is none
        for dy in (DY_MIN, np.nextafter(DY_MIN, f32(1)), np.nextafter(DY_MIN, f32(0))):
            for sx in (1.0, -1.0):
                O.append((x0, GROUND_HEIGHT + height, z0)); D.append((sx, -dy, 0.0))
    for ox in (3e38, -3e38, 1e38):   # uv * 10 overflows to +-inf: f2i(floor(inf)) saturates
        for sz in (1.0, -1.0):
            O.append((ox, GROUND_HEIGHT + 0.5, z0)); D.append((0.5, -0.01, sz))
    return np.array(O, f32), np.array(D, f32)
