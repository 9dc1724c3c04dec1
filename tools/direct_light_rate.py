"""Direct light by shadow rays to the scene's emitters: what the stages cost, and how much noise the
estimator removes.

    python tools/direct_light_rate.py [--runs 5] [--samples 16] [--width 1920 --height 1080] [--child-timeout 300]
                                      [--out profiles/r26_direct_light_rate.txt]

Timings, kernel ms as median (max - min) of `runs` calls after a warm-up call:

    table    rb_scene_emitters after an rb_update (rb_last_query_ms: flag, scan, the wait for the total, scatter) for C5's
             1 048 578 triangles and for the lamp fixture
    direct   rb_direct_light_device on the first hits of C2's --width x --height pixel centres at --samples samples: all three
             stages (rb_last_query_ms), the generator's share (rb_last_camera_rays_ms), the walk alone (rb_occluded_device on the
             same records and bounds, made by rb_light_rays), and the fold as what is left
    openness rb_openness_hemisphere_device on the same surfels and samples, radius 1e20: the yardstick -- the same kernels walk
             cosine-weighted rays to the end instead of shadow rays to a bound

Noise: rb_direct_light and rb_trace_hemisphere at max_depth = 1 under a black sky (trace_ray is then an estimator of the same
integral) on the same floor points of the Cornell box and of the lamp scene -- first hits with an upward normal at the lowest
height --, one surfel per sample so that the per-sample values come back; per point the variance of the mean of the three
channels, and the ratio of the two variances: how many times fewer samples the direct estimator needs for the same noise.
One process per scene.
"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _rate import Report, child_argv, child_exit, med_text, run_children, scene_of


def engine_of(s):
    from renderbaby_amd import Engine, RenderConfig
    rc = RenderConfig.from_scene(s)
    e = Engine.new(rc, device=0)
    e.update(rc)
    return e, rc


def table(name, runs):
    import ctypes as C
    from renderbaby_amd import Change, RenderConfig
    s = scene_of(name).with_params(width=64, height=36, spp=1)
    e, rc = engine_of(s)
    ms = []
    for run in range(runs + 1):
        e.update(RenderConfig(uniforms=Change.update(s.uniforms)))   # any accepted update: the table is made again
        count = C.c_size_t(0)   # the call that builds, on its own: Engine.scene_emitters asks twice, and the second finds the table standing
        e._check(e._lib.rb_scene_emitters(e._h, None, 0, C.byref(count)))
        if run:
            ms.append(e.last_query_ms())
        t = e.scene_emitters()
    e.close()
    kinds = {2: "triangles", 3: "spheres", 4: "lights"}
    what = ", ".join(f"{int((t['kind'] == k).sum())} {v}" for k, v in kinds.items())
    return [f"table    {name:7} {len(s.bvh_triangles):8d} triangles {len(s.spheres):4d} spheres {len(s.lights):3d} lights -> {len(t):6d} emitters ({what})  {med_text(ms)} ms"]


def stages(name, width, height, samples, runs):
    import numpy as np
    import torch
    from renderbaby_amd import abi, aov, engine
    s = scene_of(name).with_params(width=width, height=height, spp=1)
    e, _ = engine_of(s)
    _, pts, nrm = aov.ambient_occlusion_surfels(s.uniforms, e.render_hits())
    n = len(pts)
    dev = torch.device("cuda", 0)
    tp, tn = torch.from_numpy(np.ascontiguousarray(pts)).to(dev), torch.from_numpy(np.ascontiguousarray(nrm)).to(dev)
    tab = e.scene_emitters()
    recs = torch.empty((n * samples, 8), dtype=torch.float32, device=dev)
    bound = torch.empty(n * samples, dtype=torch.float32, device=dev)
    step = max(1, (1 << 22) // samples)
    for i0 in range(0, n, step):
        sl = slice(i0, min(i0 + step, n))
        rays, tmax, _ = engine.light_rays(tab, pts[sl], nrm[sl], samples, seeds=np.arange(sl.start, sl.stop, dtype=np.uint32), device=0)
        recs[sl.start * samples:sl.stop * samples] = torch.from_numpy(rays.view(np.float32).reshape(-1, 8)).to(dev)
        bound[sl.start * samples:sl.stop * samples] = torch.from_numpy(tmax).to(dev)
    out = torch.empty((n, 4), dtype=torch.float32, device=dev)
    opn = torch.empty((n, 2), dtype=torch.int32, device=dev)
    byt = torch.empty(n * samples, dtype=torch.uint8, device=dev)
    ms = {k: [] for k in ("all", "gen", "walk", "open", "open_gen")}
    for run in range(runs + 1):
        e.direct_light(tp, tn, samples, out=out)
        a, g, kernel = e.last_query_ms(), e.last_camera_rays_ms(), e.last_query_kernel_name()
        e.occluded_records(recs, bound, abi.MASK_ALL, out=byt)
        w = e.last_query_ms()
        e.openness(tp, tn, samples, 1e20, abi.MASK_ALL, out=opn)
        o, og = e.last_query_ms(), e.last_camera_rays_ms()
        if run:
            for k, v in zip(ms, (a, g, w, o, og)):
                ms[k].append(v)
    fold = [a - g - w for a, g, w in zip(ms["all"], ms["gen"], ms["walk"])]
    lit = float((out[:, :3].sum(1) > 0).float().mean().item())
    e.close()
    return [f"direct   {name:7} {n:8d} surfels x {samples:3d}, {len(tab)} emitters, {kernel}: all {med_text(ms['all'])} ms  generator {med_text(ms['gen'])}  "
            f"walk alone {med_text(ms['walk'])}  fold (the rest) {med_text(fold)}; {100 * lit:.1f} % of the surfels lit",
            f"openness {name:7} {n:8d} surfels x {samples:3d}, radius 1e20: all {med_text(ms['open'])} ms  generator {med_text(ms['open_gen'])}"]


def noise(name, points, samples):
    import numpy as np
    from renderbaby_amd import aov
    s = scene_of(name).with_params(width=96, height=54, spp=1, max_depth=1)
    s.uniforms["sky_color"] = (0, 0, 0)
    e, _ = engine_of(s)
    _, pts, nrm = aov.ambient_occlusion_surfels(s.uniforms, e.render_hits())
    up = nrm[:, 1] > 0.99
    floor = up & (pts[:, 1] < pts[up, 1].min() + 1e-3)
    idx = np.nonzero(floor)[0]
    idx = idx[(np.arange(min(points, len(idx))) * len(idx)) // min(points, len(idx))]
    p, nn = np.repeat(pts[idx], samples, axis=0), np.repeat(nrm[idx], samples, axis=0)
    h = e.trace_hemisphere(p, nn, 1)["sum"].astype(np.float64).mean(1).reshape(len(idx), samples)
    d = e.direct_light(p, nn, 1)["sum"].astype(np.float64).mean(1).reshape(len(idx), samples)
    n_emit = len(e.scene_emitters())
    e.close()
    vh, vd = h.var(1, ddof=1), d.var(1, ddof=1)
    ok = (vh > 0) & (vd > 0)
    ratio = vh[ok] / vd[ok]
    return [f"noise    {name:7} {len(idx):3d} floor points x {samples} samples, {n_emit} emitters: mean hemisphere {h.mean():.4f} direct {d.mean():.4f}; "
            f"per-point variance hemisphere / direct: median {np.median(ratio):8.1f}  min {ratio.min():8.1f}  max {ratio.max():8.1f}  "
            f"({int(ok.sum())} points with light in both); pooled {vh.mean() / vd.mean():8.1f}"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--noise-points", type=int, default=64)
    ap.add_argument("--noise-samples", type=int, default=1024)
    ap.add_argument("--child-timeout", type=int, default=300, help="seconds one child process may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        kind, name = a.child.split(":")
        lines = (table(name, a.runs) if kind == "table" else stages(name, a.width, a.height, a.samples, a.runs) if kind == "stages"
                 else noise(name, a.noise_points, a.noise_samples))
        print("\n".join(lines), flush=True)
        child_exit()
    from renderbaby_amd._lib import source_fingerprint   # (this process never opens the device: the children do)
    with Report(a.out) as r:
        r.say(f"# library sources {source_fingerprint()}; kernel ms as median (max - min) of {a.runs} calls after a warm-up call; one process per line group")
        r.say("# table: rb_scene_emitters after an rb_update (flag, scan, the wait for the total, scatter); direct: rb_direct_light_device, its generator's")
        r.say("# share, rb_occluded_device alone on the same records and bounds, the fold as the rest; openness: rb_openness_hemisphere_device, the yardstick")
        r.say("# noise: max_depth = 1, black sky, one surfel per sample; variance of the per-sample mean of the three channels, per floor point")
        options = ("runs", "samples", "width", "height", "noise_points", "noise_samples")
        ok, _ = run_children(r, lambda name, first: child_argv(__file__, name, a, options),
                             ("table:c5", "table:lamp", "stages:c2", "noise:cornell", "noise:lamp"), a.child_timeout)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
