"""Direct light with a weighted pick: what the pick by a table costs beside the uniform pick, what the
table costs to make, and how much noise the pick by power removes.

    python tools/direct_pick_rate.py [--runs 5] [--samples 16] [--width 1920 --height 1080] [--child-timeout 300]
                                     [--out profiles/r35_direct_pick_rate.txt]

Timings, kernel ms as median (max - min) of `runs` calls after a warm-up call, both picks in one process on the same surfels
and samples -- the uniform pick, rb_direct_light_device as it always was, is the yardstick:

    direct   rb_direct_light_device against rb_direct_light_cdf_device with the scene's kept table: all three stages
             (rb_last_query_ms) and the generator's share (rb_last_camera_rays_ms), on C2's first hits (2 emitters) and on the
             ground hits of spheres_scene(n = 10^6) (about 10^4 emitters; two lights are added, so its table has both arms)
    table    rb_scene_emitter_cdf after an rb_update and rb_scene_emitters (rb_last_query_ms: the powers and their maximum, the
             quantised weights, the scan) for both tables

Noise, by direct_light_rate.py's method: one surfel per sample so that the per-sample values come back; per point the variance
of the mean of the three channels under either pick, and the ratio uniform / power, on ground points of
spheres_scene(n = 100 000) (993 emitters) and on 8 floor points of the feature scene (5 emitters).  One process per scene.
"""
import argparse, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _rate import Report, child_argv, child_exit, med_text, run_children, scene_of


def spheres(n, with_lights=False):
    import numpy as np
    from renderbaby_amd import abi, scenes
    s = scenes.spheres_scene(n=n)
    if not with_lights:
        return s
    lights = np.zeros(2, dtype=abi.POINT_LIGHT)   # the sphere arm twice over: the table then has two kinds
    lights["center"], lights["radius"] = [(-30.0, 40.0, 0.0), (30.0, 40.0, -5.0)], (1.0, 0.5)
    lights["material"]["emissive"] = [(50.0, 40.0, 30.0), (10.0, 20.0, 30.0)]
    return scenes.Scene(s.uniforms, s.spheres, lights, s.meshes, s.bvh_nodes, s.bvh_indices, s.bvh_triangles, s.uvs, name="c4 with lights")


OWN = {"c4": lambda: spheres(1_000_000, with_lights=True), "c4like": lambda: spheres(100_000)}   # (not the table's c4)


def engine_of(s):
    from renderbaby_amd import Engine, RenderConfig
    rc = RenderConfig.from_scene(s)
    e = Engine.new(rc, device=0)
    e.update(rc)
    return e, rc


def ground(pts, nrm):
    """which surfels lie on the lowest upward-facing level"""
    up = nrm[:, 1] > 0.99
    return up & (pts[:, 1] < pts[up, 1].min() + 1e-3)


def stages(name, width, height, samples, runs):
    import ctypes as C
    import numpy as np
    import torch
    from renderbaby_amd import Change, RenderConfig, aov
    s = scene_of(name, OWN).with_params(width=width, height=height, spp=1)
    e, _ = engine_of(s)
    _, pts, nrm = aov.ambient_occlusion_surfels(s.uniforms, e.render_hits())
    if name == "c4":
        keep = ground(pts, nrm)
        pts, nrm = pts[keep], nrm[keep]
    n = len(pts)
    dev = torch.device("cuda", 0)
    tp, tn = torch.from_numpy(np.ascontiguousarray(pts)).to(dev), torch.from_numpy(np.ascontiguousarray(nrm)).to(dev)
    tab = e.scene_emitters()
    kinds = {2: "triangles", 3: "spheres", 4: "lights"}
    what = ", ".join(f"{int((tab['kind'] == k).sum())} {v}" for k, v in kinds.items())
    out = torch.empty((n, 4), dtype=torch.float32, device=dev)
    ms = {k: [] for k in ("uni", "uni_gen", "pow", "pow_gen", "build")}
    for run in range(runs + 1):
        e.update(RenderConfig(uniforms=Change.update(s.uniforms)))   # any accepted update: both tables are made again
        count = C.c_size_t(0)
        e._check(e._lib.rb_scene_emitters(e._h, None, 0, C.byref(count)))
        e._check(e._lib.rb_scene_emitter_cdf(e._h, None, 0, C.byref(count)))   # the call that builds, on its own
        b = e.last_query_ms()
        e.direct_light(tp, tn, samples, out=out)
        u, ug, kernel = e.last_query_ms(), e.last_camera_rays_ms(), e.last_query_kernel_name()
        e.direct_light(tp, tn, samples, out=out, pick="power")
        p, pg = e.last_query_ms(), e.last_camera_rays_ms()
        if run:
            for k, v in zip(ms, (u, ug, p, pg, b)):
                ms[k].append(v)
    cdf = e.scene_emitter_cdf()
    e.close()
    share = lambda g, a: 100 * statistics.median(g) / statistics.median(a)
    return [f"direct   {name:7} {n:8d} surfels x {samples:3d}, {len(tab)} emitters ({what}), {kernel}:",
            f"         uniform  all {med_text(ms['uni'])} ms  generator {med_text(ms['uni_gen'])}  ({share(ms['uni_gen'], ms['uni']):.1f} % of the call)",
            f"         by power all {med_text(ms['pow'])} ms  generator {med_text(ms['pow_gen'])}  ({share(ms['pow_gen'], ms['pow']):.1f} % of the call); "
            f"generator x {statistics.median(ms['pow_gen']) / statistics.median(ms['uni_gen']):.2f}, call x {statistics.median(ms['pow']) / statistics.median(ms['uni']):.3f}",
            f"table    {name:7} rb_scene_emitter_cdf of {len(cdf)} emitters, total {int(cdf[-1]) if len(cdf) else 0}: {med_text(ms['build'])} ms"]


def noise(name, points, samples):
    import numpy as np
    from renderbaby_amd import aov, direct
    s = scene_of(name, OWN)
    if name == "feature":
        pts = np.array([(x, -1.0, z) for x in (-1.5, 0.5) for z in (-3.0, -2.0, -1.0, 0.0)], np.float32)
        nrm = np.tile(np.float32([0, 1, 0]), (len(pts), 1))
        e, _ = engine_of(s)
    else:
        s = s.with_params(width=96, height=54, spp=1)
        e, _ = engine_of(s)
        _, p0, n0 = aov.ambient_occlusion_surfels(s.uniforms, e.render_hits())
        idx = np.nonzero(ground(p0, n0))[0]
        idx = idx[(np.arange(min(points, len(idx))) * len(idx)) // min(points, len(idx))]
        pts, nrm = p0[idx], n0[idx]
    p, nn = np.repeat(pts, samples, axis=0), np.repeat(nrm, samples, axis=0)
    u = e.direct_light(p, nn, 1)["sum"].astype(np.float64).mean(1).reshape(len(pts), samples)
    w = e.direct_light(p, nn, 1, pick="power")["sum"].astype(np.float64).mean(1).reshape(len(pts), samples)
    power = direct.emitter_weights(e.scene_emitters())
    e.close()
    vu, vw = u.var(1, ddof=1), w.var(1, ddof=1)
    ok = (vu > 0) & (vw > 0)
    ratio = vu[ok] / vw[ok]
    se = np.hypot(u.std(ddof=1), w.std(ddof=1)) / np.sqrt(u.size)
    return [f"noise    {name:7} {len(pts):3d} points x {samples} samples, {len(power)} emitters of power {power.min():.3g} .. {power.max():.3g}: "
            f"mean uniform {u.mean():.5f} by power {w.mean():.5f} ({abs(u.mean() - w.mean()) / se:.2f} combined standard errors apart)",
            f"         per-point variance uniform / power: " + " ".join(f"{r:.2f}" for r in ratio) + f"  ({int(ok.sum())} points with light); pooled {vu.mean() / vw.mean():.2f}"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--child-timeout", type=int, default=300, help="seconds one child process may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        kind, name = a.child.split(":")
        lines = (stages(name, a.width, a.height, a.samples, a.runs) if kind == "stages"
                 else noise(name, 6, 65536) if name == "c4like" else noise(name, 8, 4096))
        print("\n".join(lines), flush=True)
        child_exit()
    from renderbaby_amd._lib import source_fingerprint   # (this process never opens the device: the children do)
    with Report(a.out) as r:
        r.say(f"# library sources {source_fingerprint()}; kernel ms as median (max - min) of {a.runs} calls after a warm-up call; one process per line group")
        r.say("# direct: rb_direct_light_device (uniform, the yardstick) and rb_direct_light_cdf_device with the scene's kept table (by power) on the same")
        r.say("# surfels and samples, all three stages and the generator's share; table: rb_scene_emitter_cdf after an rb_update and rb_scene_emitters")
        r.say("# noise: one surfel per sample; variance of the per-sample mean of the three channels under either pick, per point")
        ok, _ = run_children(r, lambda name, first: child_argv(__file__, name, a, ("runs", "samples", "width", "height")),
                             ("stages:c2", "stages:c4", "noise:c4like", "noise:feature"), a.child_timeout)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
