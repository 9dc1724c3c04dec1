"""What the tests of the triangle sift share (tests/test_tri_filter_model.py on the CPU, tests/test_gpu_tri_filter.py on the
device): the float32 reference test of tools/margin_check.py, a scene's table and region from the numpy model
(renderbaby_amd/tri_filter_model.py), the accepted slots of a set of rays, and ray families."""
import importlib.util
import os

import numpy as np

from renderbaby_amd import scenes
from renderbaby_amd import tri_filter_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MC = _tool("margin_check")


MC = _tool("margin_check")


def _prepared(scene):
    t = scene.bvh_triangles[scene.bvh_indices]
    v0 = t["v0"].astype(F32)
    return v0, t["v1"].astype(F32) - v0, t["v2"].astype(F32) - v0


def _scene_table(scene, origins=None):
    """the scene's table and the region of a launch over it; `origins`: rays start there as if the camera did (their finite box joins)"""
    v0, e1, e2 = _prepared(scene)
    assert len(v0) <= M.MAX_SLOTS
    groups, live, closed = M.build_table(v0, e1, e2, np.ones(len(v0), bool))
    cam = np.asarray(scene.uniforms["camera"]["pos"][0], np.float64)
    lo, hi = cam.copy(), cam.copy()
    for s in scene.spheres:
        r = abs(float(s["radius"])) * 1.0001
        lo, hi = np.minimum(lo, s["center"] - r), np.maximum(hi, s["center"] + r)
    if origins is not None:
        o = np.asarray(origins, np.float64)
        o = o[np.all(np.abs(o) < 1e6, axis=1)]
        lo, hi = np.minimum(lo, o.min(0)), np.maximum(hi, o.max(0))
    return groups, M.table_region(groups, lo, hi), (v0, e1, e2)


def _accepted(tri, o, d):
    v0, e1, e2 = tri
    out = np.zeros((len(v0), o.shape[1]), bool)
    for k in range(len(v0)):
        with np.errstate(all="ignore"):   # (the families carry infinite and NaN components on purpose)
            ok, _, _ = MC.mt32(tuple(o), tuple(d), *(tuple(np.full(o.shape[1], a[k][i], F32) for i in range(3)) for a in (v0, e1, e2)))
        out[k] = ok
    return out


def _hold(scene_table, o, d, what):
    groups, reg, tri = scene_table
    o, d = np.ascontiguousarray(np.asarray(o, F32).T), np.ascontiguousarray(np.asarray(d, F32).T)
    cand, acc = M.candidate_mask(groups, reg, o, d), _accepted(tri, o, d)
    print(f"{what}: {o.shape[1]} rays, {int(acc.sum())} accepted hits, candidates per ray mean {cand.sum(0).mean():.2f} max {int(cand.sum(0).max())}")
    assert not (acc & ~cand).any(), (what, int((acc & ~cand).sum()))
    return cand, acc


def _unit(d):
    d = np.asarray(d, F32)
    with np.errstate(all="ignore"):
        return (d / np.sqrt((d * d).sum(1, dtype=F32))[:, None]).astype(F32)


def tiny_component_rays(n_per=24, seed=9):
    """Origins inside the Cornell box, directions with one or two components swept over the smallest normal exponents and the
    subnormals beside them (+-2^-149 .. 2^-100), the others of ordinary size -> (o [n][3], d [n][3]) float32.  1 / d_k is then
    finite and up to 2^126, or infinite."""
    rng = np.random.default_rng(seed)
    b = scenes.BOX
    lo, hi = np.array([b["x0"], b["y0"], b["z0"]]), np.array([b["x1"], b["y1"], b["z1"]])
    tiny = [s * m * 2.0 ** e for e in list(range(-149, -99, 2)) + [-127, -126, -125] for m in (1.0, 1.2, 1.9999999) for s in (1.0, -1.0)]
    O, D = [], []
    for t in tiny:
        for k in range(3):
            for two in (False, True):
                d = rng.normal(size=(n_per, 3))
                d[:, k] = t
                if two:
                    d[:, (k + 1) % 3] = -t
                O.append(lo + rng.random((n_per, 3)) * (hi - lo))
                D.append(d)
    o, d = np.concatenate(O).astype(F32), np.concatenate(D).astype(F32)
    keep = np.abs(d).max(1) > 0.05     # (an ordinary component beside the tiny ones)
    return o[keep], d[keep]
