"""The two numbers the triangle sift's estimate rests on, counted on a sample of C2's rays with the
device's own pass 1 (rb_debug_tri_filter): candidates per lane, and trips of pass 2 per iteration of a wavefront -- pass 2 is a
wave loop, so it runs as many trips as its busiest lane has candidates.

The sample: paths of the C2 scene followed on the host with the closest-hit query (Engine.cast_rays) -- pixel-centre primaries of
a grid of pixels, then up to max_depth segments each, scattered as the materials do (a mirror direction for the metals, normal +
unit vector for the others; a path ends at the light, at nothing, or at the depth).  Not the renderer's paths sample for sample,
but its population of segments: origins on the walls, the spheres and the camera, directions over the hemispheres.  Wavefronts
are formed two ways: 64 segments of neighbouring pixels at the same depth (a wave right after a refill) and 64 segments drawn from
the whole population (a wave whose lanes have been refilled at different times), which is what the persistent loop tends to.

    python tools/tri_filter_stats.py [pixels per axis, default 192] > profiles/rNN_tri_filter_stats.txt      (needs the GPU)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from renderbaby_amd import Engine, RenderConfig, abi, scenes  # noqa: E402


def unit(v):
    return v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-30)


def main():
    n_axis = int(sys.argv[1]) if len(sys.argv) > 1 else 192
    scene = scenes.cornell_c2()
    depth = int(scene.uniforms["max_depth"][0])
    rc = RenderConfig.from_scene(scene.with_params(width=64, height=48, spp=1))
    e = Engine.new(rc, queue_batch=256)
    e.update(rc)
    rng = np.random.default_rng(33)
    cam = scene.uniforms["camera"][0]
    pos, fwd = np.asarray(cam["pos"], np.float64), np.asarray(cam["dir"], np.float64)
    right = unit(np.cross(fwd, [0.0, 1.0, 0.0])[None])[0]
    up = np.cross(right, fwd)
    xs, ys = np.meshgrid((np.arange(n_axis) + 0.5) / n_axis - 0.5, (np.arange(n_axis) + 0.5) / n_axis - 0.5)
    aspect = 1920.0 / 1080.0
    d = fwd[None] * float(cam["pane_distance"]) + right[None] * (xs.reshape(-1, 1) * float(cam["pane_width"])) + \
        up[None] * (ys.reshape(-1, 1) * float(cam["pane_width"]) / aspect)
    o, d = np.tile(pos, (len(d), 1)), unit(d)
    alive = np.ones(len(o), bool)
    seg_o, seg_d, seg_depth, seg_pix = [], [], [], []
    for k in range(depth):
        idx = np.flatnonzero(alive)
        if len(idx) == 0:
            break
        seg_o.append(o[idx].astype(np.float32)), seg_d.append(d[idx].astype(np.float32))
        seg_depth.append(np.full(len(idx), k)), seg_pix.append(idx)
        hits, surf = e.cast_rays(o[idx].astype(np.float32), d[idx].astype(np.float32), surfaces=True)
        hit = (hits["kind"] == abi.HIT_TRIANGLE) | (hits["kind"] == abi.HIT_SPHERE)
        lit = surf["emissive"].sum(1) > 0
        go = hit & ~lit
        p = o[idx] + hits["t"][:, None].astype(np.float64) * d[idx]
        nrm = hits["normal"].astype(np.float64)
        metal = (surf["flags"] & abi.SURFACE_IS_METAL) != 0
        refl = d[idx] - 2.0 * (d[idx] * nrm).sum(1, keepdims=True) * nrm
        nd = np.where(metal[:, None], refl, nrm + unit(rng.normal(size=nrm.shape)))
        o[idx], d[idx] = p, unit(nd)
        alive[idx] = go
    O, D, K, P = (np.concatenate(a) for a in (seg_o, seg_d, seg_depth, seg_pix))
    masks, first = e.tri_filter_masks(O, D)
    e.close()
    cand = masks.sum(0)
    print(f"# tri_filter_stats: C2's scene, {n_axis} x {n_axis} pixel centres followed to depth {depth} on the host with rb_cast_rays: {len(O)} segments, "
          f"{len(O) / (n_axis * n_axis):.3f} per path (the renderer counts 5.155); candidate masks by rb_debug_tri_filter, {masks.shape[0]} slots")
    print("candidates per lane: mean %.3f;  share of lanes with 0, 2, 4, 6, 8+ : %s" %
          (cand.mean(), "  ".join(f"{k}{'+' if k == 8 else ''}: {((cand >= 8) if k == 8 else (cand == k)).mean():.4f}" for k in (0, 2, 4, 6, 8))))
    print("  by depth of the segment: " + "  ".join(f"{k}: {cand[K == k].mean():.3f}" for k in range(depth) if (K == k).any()))
    odd = (cand % 2 == 1).mean()
    print(f"  (an odd count -- one triangle of a quad without the other -- in {odd:.5f} of the lanes: a group's bit goes to both members)")

    def trips(order, what):
        n = len(order) // 64 * 64
        t = cand[order[:n]].reshape(-1, 64).max(1)
        print(f"pass-2 trips per wave-iteration, {what}: mean {t.mean():.3f};  share of iterations with 2, 4, 6, 8+ trips: " +
              "  ".join(f"{k}{'+' if k == 8 else ''}: {((t >= 8) if k == 8 else (t == k)).mean():.4f}" for k in (2, 4, 6, 8)) +
              f";  mean candidates in such a wave {cand[order[:n]].reshape(-1, 64).sum(1).mean():.1f} of {64 * masks.shape[0]}")
        return t.mean()

    trips(np.lexsort((P, K)), "64 neighbouring pixels at one depth")
    mixed = trips(rng.permutation(len(O)), "64 segments drawn from the whole population")
    print(f"# the estimate of the issue assumed about 4 trips; tools/ktrace_budget.py prices pass 2 with the mixed figure, {mixed:.2f}")


if __name__ == "__main__":
    main()
